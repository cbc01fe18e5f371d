"""The recurrent actor-critic's whole update on the MI355X (``RecurrentConfig(update_through_time="hip", update_heads="hip")``;
mpc_ppo_update_set_sequence_rows, mpc_ppo_update_grads_sequence, mpc_ppo_update_bind_extra of include/mpc_ppo_update.h; pgemm::kBackwardDataLinear).

Bit for bit: the MLPs' half of ``mpc_ppo_update_grads_sequence`` against ``mpc_ppo_update_grads`` on a feed-forward asymmetric actor-critic with the
same weights over the gathered block (identity index); the memories' gradients against ``SequenceKernel.backward`` fed the two dY buffers;
``mpc_ppo_update_apply`` after ``bind_extra(count=0)`` against today's; reruns; sentinel rows; a smaller mini-batch on a used handle.

Against float64: the new GEMM kind element by element within gamma_{K+2} sum |dy w| (tests/test_ppo_gemm_gpu.py's derivation: K products, and the
bound is asserted to bite); the whole update under DESIGN section 8.3.4's rule -- `gap` is the distance of torch's float32 CPU autograd from the float64
restatement (tests/recurrent_update_ref.py) on the same inputs, and a device quantity may be off torch's float32 by 4 x gap.  The shapes are
tests/test_recurrent_update.py's tables, whose plan test pins which kernels they reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, ppo as P, privileged_obs as V, recurrent as RC, rl_task as R
from tests import ppo_update_ref as ref
from tests import recurrent_update_ref as uref
from tests import test_recurrent_update as cases
from tests.helpers import ROOT, draw, gamma
from tests.test_ppo_gemm_gpu import Launch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "device", "ppo_gemm_linear_harness.hip")
HIPCC = "/opt/rocm/bin/hipcc"
PAD, SENTINEL = 16, 12345.0
RATIOS = {}                                                       # what -> largest error / gap seen, printed as evidence


def _ids(case):
    I, H, nets, T, N, mb, wp = case
    return f"I{I}-H{H}-{len(nets[0])}x{nets[0][0]}-T{T}-N{N}-mb{mb}" + (f"-priv{wp}" if wp else "")


def _cfg(case, **kw):
    nets, mb = case[2], case[5]
    kw.setdefault("num_learning_epochs", 1)
    return P.PPOConfig(actor_hidden_dims=nets[0], critic_hidden_dims=nets[1], init_noise_std=0.7, num_mini_batches=mb, **kw)


def _to_device(ac, st):
    """The storage on the device, and ``ac`` (made on the CPU with the device options) moved there."""
    out = P.RolloutStorage(st.n, st.T, DEV, num_obs=st.observations.shape[-1],
                           num_privileged_obs=None if st.privileged_observations is None else st.privileged_observations.shape[-1], hidden=st.hidden)
    for k, v in list(vars(st).items()):
        if torch.is_tensor(v):
            getattr(out, k).copy_(v)
    out.step = out.T
    return ac.to(DEV), out


_FIXTURES = {}


def _fixture(case, realistic=None):
    """(CPU actor-critic, CPU storage) of a case, made once and never changed."""
    if case not in _FIXTURES:
        I, H, nets, T, N, mb, wp = case
        cpu, _ = uref.recurrent_pair(I, H, nets, seed=5, critic_width=wp)
        _FIXTURES[case] = (cpu, uref.filled_storage(cpu, T, N, seed=6, realistic=case != cases.PRODUCTION if realistic is None else realistic))
    return _FIXTURES[case]


def _device(case, **cfg_kw):
    """(device actor-critic with both options, device storage, PPO over it) with the fixture's weights and rows."""
    I, H, nets, T, N, mb, wp = case
    cpu, st = _fixture(case)
    _, dev = uref.recurrent_pair(I, H, nets, seed=5, critic_width=wp, update_through_time="hip", update_heads="hip")
    dev, dst = _to_device(dev, st)
    return dev, dst, P.PPO(dev, _cfg(case, **cfg_kw))


def _guarded(rows, width):
    buf = torch.full(((rows + 2 * PAD) * width,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[PAD * width:(PAD + rows) * width].view(rows, width)


def _intact(buf, rows, width):
    return bool((buf[:PAD * width] == SENTINEL).all()) and bool((buf[(PAD + rows) * width:] == SENTINEL).all())


def _grads_of(alg, dst, i, lr=1e-3):
    """Mini-batch i up to the gradients -> (plan, {name: .grad}, terms [4], learning rate, the four dense buffers), all cloned, on the host."""
    plan = alg._recurrent_plan(dst)
    alg.lr_device.fill_(lr)
    terms = torch.zeros(4, device=DEV)
    alg._recurrent_grads(plan, i, terms)
    torch.cuda.synchronize()
    return (plan, {k: p.grad.detach().cpu().clone() for k, p in alg.actor_critic.named_parameters()}, terms.cpu().clone(), float(alg.lr_device),
            [t.detach().cpu().clone() for t in alg._seq_rows])


SMALL_TENSOR = 16


def _small_gap(sides):
    """A tensor of a few elements (std, the last layers' biases: 12, 12 and 1) has a float32 gap of a few rounding draws, which can be next to nothing
    (tests/test_ppo_update.py pools its scalars for that reason): such tensors share the largest of their gaps, each relative to its tensor's largest
    float64 element, over all mini-batches of the case.  ``sides``: (g64, g32) dicts per mini-batch."""
    return max(float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max()) for g64, g32 in sides for k in g64 if g64[k].numel() < SMALL_TENSOR)


def _gap_rule(got, t32, t64, what, key=None, small_gap=None):
    """Section 8.3.4's rule on one tensor: the device may be off torch's float32 by 4 x torch's own distance from float64, the distance being the
    largest element difference over the tensor (``small_gap``, for a tensor under SMALL_TENSOR elements: ``_small_gap``'s pooled one)."""
    g, a, b = (t.detach().double().cpu().reshape(-1) for t in (got, t32, t64))
    gap, d = float((a - b).abs().max()), float((g - a).abs().max())
    if small_gap is not None and g.numel() < SMALL_TENSOR:
        own = d / gap if gap > 0 else float("inf")
        gap = small_gap * float(b.abs().max())
        print(f"{what}: {g.numel()} elements, error / its own gap {own:.3f} (own gap {float((a - b).abs().max()):.3e}, pooled gap {gap:.3e})")
        RATIOS["small tensors against their own gap"] = max(RATIOS.get("small tensors against their own gap", 0.0), own)
    ratio = d / gap if gap > 0 else (0.0 if d == 0 else float("inf"))
    print(f"{what}: off torch's float32 by {d:.3e}, gap {gap:.3e}, ratio {ratio:.3f} (bound 4)")
    if key is not None:
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    assert d <= 4 * gap, f"{what}: off by {d:.3e} > 4 x {gap:.3e}"


# ---- 1. the new GEMM kind against float64, element by element -------------------------------------------------------------------------------------------------
LINEAR_SHAPES = (((85, 16, 32), (85, 16, 64)), ((260, 16, 32), None), ((51, 256, 32), (51, 256, 64)), ((129, 65, 33), (33, 12, 240)), ((1, 128, 1), (257, 144, 100)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("ppo_gemm_linear_harness") / "ppo_gemm_linear_harness.so"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, HARNESS, "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.ppo_gemm_linear_harness_sizeof_launch.restype = C.c_int
    L.ppo_gemm_linear_harness_launch.argtypes = [C.POINTER(Launch), C.c_int, C.c_void_p]; L.ppo_gemm_linear_harness_launch.restype = C.c_int
    assert L.ppo_gemm_linear_harness_sizeof_launch() == C.sizeof(Launch)
    return L


@pytest.mark.parametrize("wide", (0, 1), ids=("narrow", "wide"))
def test_linear_backward_data_against_float64(harness, wide):
    """dX = dY W with no factor, (M, N, K) of LINEAR_SHAPES (the update's own first layers at the test cases' rows, tile and vector edges), two problems
    per launch and one empty slot.  Operands have NaN in their padding columns; the output is pre-filled with a sentinel that must survive outside M x N."""
    rng = np.random.default_rng(17)
    worst = 0.0
    for shapes in LINEAR_SHAPES:
        L, keep, checks = Launch(), [], []
        for slot, s in enumerate(shapes):
            if s is None:
                continue
            M, N, K = s
            lda, ldb, ldc = (K + 3) // 4 * 4 + 4, (N + 3) // 4 * 4 + 4, (N + 3) // 4 * 4 + 4
            dY, W = np.full((M, lda), np.nan, np.float32), np.full((K, ldb), np.nan, np.float32)
            dY[:, :K], W[:, :N] = draw(rng, (M, K), 0.1), draw(rng, (K, N), 0.7)
            exact = dY[:, :K].astype(np.float64) @ W[:, :N].astype(np.float64)
            sabs = np.abs(dY[:, :K]).astype(np.float64) @ np.abs(W[:, :N]).astype(np.float64)
            bound = gamma(K + 2) * sabs
            min_term = np.outer(np.abs(dY[:, :K]).min(1), np.abs(W[:, :N]).min(0))
            assert (min_term >= 3.0 * bound).all(), (s, float((min_term / bound).min()))      # a dropped, doubled or misplaced term cannot pass
            d_dY, d_W = torch.from_numpy(dY).to(DEV), torch.from_numpy(W).to(DEV)
            out = torch.full((M + 2 * PAD, ldc), SENTINEL, dtype=torch.float32, device=DEV)
            keep += [d_dY, d_W, out]
            p = L.p[slot]
            p.A, p.B, p.C = d_dY.data_ptr(), d_W.data_ptr(), out[PAD:].data_ptr()
            p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.chunks = M, N, K, lda, ldb, ldc, 1
            p.tiles_m, p.tiles_n = (M + 127) // 128, (N + (128 if wide else 64) - 1) // (128 if wide else 64)
            checks.append((s, out, exact, bound))
        assert harness.ppo_gemm_linear_harness_launch(C.byref(L), wide, None) == 0
        torch.cuda.synchronize()
        for (M, N, K), out, exact, bound in checks:
            got = out.cpu().numpy()
            assert (got[:PAD] == SENTINEL).all() and (got[PAD + M:] == SENTINEL).all() and (got[PAD:PAD + M, N:] == SENTINEL).all(), (M, N, K)
            err = np.abs(got[PAD:PAD + M, :N].astype(np.float64) - exact)
            assert (err <= bound).all(), ((M, N, K), float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
    print(f"linear backward data, {'wide' if wide else 'narrow'} tile: largest error / bound {worst:.3f}")


# ---- 2. bit for bit against the feed-forward update and the roll's own backward pass ---------------------------------------------------------------------------
def _feed_forward_grads(case, dev, dst, y_a, y_c, i, cfg):
    """``mpc_ppo_update_grads`` on a feed-forward asymmetric ActorCritic(H, num_critic_obs=H) with dev's MLP weights, whose flat storage is block i
    gathered, observations = y_a, privileged_observations = y_c, through the identity index."""
    I, H, nets, T, N, mb, wp = case
    B = N // mb
    rows, e0 = T * B, i * B
    ff = P.ActorCritic(H, 12, *nets, init_noise_std=0.7, num_critic_obs=H)
    ff.load_state_dict({k: v.detach().cpu() for k, v in dev.state_dict().items() if not k.startswith("memory_")})
    ff = ff.to(DEV)
    fst = P.RolloutStorage(B, T, DEV, num_obs=H, num_privileged_obs=H)
    fst.observations.copy_(y_a.view(T, B, H)); fst.privileged_observations.copy_(y_c.view(T, B, H))
    for f in ref.FIELDS[1:]:
        getattr(fst, f).copy_(getattr(dst, f)[:, e0:e0 + B])
    alg = P.PPO(ff, cfg, backend="hip")
    alg._device_state(rows)
    L = P.update_lib()
    P.check(L.mpc_ppo_update_set_storage(alg._handle, rows, *[getattr(fst, f).data_ptr() for f in ref.FIELDS]), "set_storage")
    P.check(L.mpc_ppo_update_set_critic_storage(alg._handle, fst.privileged_observations.data_ptr()), "set_critic_storage")
    idx = torch.arange(rows, dtype=torch.long, device=DEV)
    terms = torch.zeros(4, device=DEV)
    alg.lr_device.fill_(1e-3)
    c = alg.cfg
    P.check(L.mpc_ppo_update_grads(alg._handle, rows, idx.data_ptr(), c.clip_param, c.value_loss_coef, c.entropy_coef, int(c.use_clipped_value_loss), 1,
                                   c.desired_kl, alg.lr_device.data_ptr(), terms.data_ptr(), None), "grads")
    torch.cuda.synchronize()
    return {k: p.grad.detach().cpu().clone() for k, p in ff.named_parameters()}, terms.cpu(), float(alg.lr_device)


@pytest.mark.parametrize("case", cases.CASES, ids=_ids)
def test_grads_sequence_bit_for_bit(case):
    """Per mini-batch: the MLPs' and std's gradients, the four terms and the learning-rate decision equal the feed-forward call's; the eight memory
    gradients equal a second ``SequenceKernel``'s backward pass fed the two dY buffers; the sentinel rows around the four dense buffers survive; the
    storage is not written; a rerun is identical."""
    I, H, nets, T, N, mb, wp = case
    B = N // mb
    rows = T * B
    dev, dst, alg = _device(case, desired_kl=0.06)
    before = {k: v.clone() for k, v in vars(dst).items() if torch.is_tensor(v)}
    guards = [_guarded(rows, H) for _ in range(4)]
    alg._seq_rows = tuple(v for _, v in guards)
    for i in range(mb):
        plan, got, terms, lr, (y_a, y_c, dy_a, dy_c) = _grads_of(alg, dst, i)
        assert plan["rows"] == rows and alg._seq_rows[0].data_ptr() == guards[0][1].data_ptr()
        assert all(_intact(buf, rows, H) for buf, _ in guards), "a sentinel row was written"
        want_idx = (torch.arange(T)[:, None] * N + i * B + torch.arange(B)[None, :]).reshape(-1)
        assert torch.equal(plan["idx"][i].cpu(), want_idx) and plan["idx"].shape == (mb, rows)
        want, ff_terms, ff_lr = _feed_forward_grads(case, dev, dst, y_a.to(DEV), y_c.to(DEV), i, alg.cfg)
        assert len(want) + 8 == len(got) and all(torch.equal(got[k], want[k]) for k in want), [k for k in want if not torch.equal(got[k], want[k])]
        assert torch.equal(terms, ff_terms) and lr == ff_lr
        assert all(float(got[k].abs().max()) > 0 for k in got) and float(dy_a.abs().max()) > 0 and float(dy_c.abs().max()) > 0
        # the memories: a kernel of its own over the same parameters, the same roll, fed the dY buffers
        other = RC.SequenceKernel(dev.memories())
        e0 = i * B
        critic_rows = dst.observations if wp is None else dst.privileged_observations
        ys = other.forward((0, 1), (dst.observations[:, e0:e0 + B], critic_rows[:, e0:e0 + B]), [dst.saved_h_a[0, e0:e0 + B], dst.saved_h_c[0, e0:e0 + B]],
                           [dst.saved_c_a[0, e0:e0 + B], dst.saved_c_c[0, e0:e0 + B]], plan["reset"][i])
        assert torch.equal(ys[0].cpu().view(rows, H), y_a) and torch.equal(ys[1].cpu().view(rows, H), y_c)
        mg = other.backward((0, 1), T, B, [dy_a.to(DEV), dy_c.to(DEV)])
        for name, g4 in zip(("memory_a", "memory_c"), mg):
            for key, g in zip(uref.MEMORY_KEYS, g4):
                assert torch.equal(g.cpu(), got[f"{name}.rnn.{key}"]), (name, key)
        again = _grads_of(alg, dst, i)
        assert all(torch.equal(again[1][k], got[k]) for k in got) and torch.equal(again[2], terms) and again[3] == lr
        assert all(torch.equal(a, b) for a, b in zip(again[4], (y_a, y_c, dy_a, dy_c)))
    assert all(torch.equal(getattr(dst, k), v) for k, v in before.items()), "the storage was written"


@pytest.mark.parametrize("case", [cases.SMALL[5], cases.PRIVILEGED, cases.WIDE_STATE], ids=_ids)
def test_row_gradients_are_the_first_layers_gradient_times_its_weights(case):
    """The two dY buffers ``grads_sequence`` wrote, element by element against the float64 product of the float32 dY_0 it left in the workspace
    (``mpc_ppo_update_layer_gradient``) and W_0, within gamma_{K+2} sum |dy w| (K = the first layer's width): the wiring of the launch's operands."""
    I, H, nets, T, N, mb, wp = case
    rows = T * (N // mb)
    dev, dst, alg = _device(case, desired_kl=0.06)
    L = P.update_lib()
    worst = 0.0
    for i in range(mb):
        _, _, _, _, (_, _, dy_a, dy_c) = _grads_of(alg, dst, i)
        for net, (seq, dy) in enumerate(((dev.actor, dy_a), (dev.critic, dy_c))):
            W0 = dev._linears(seq)[0].weight.detach().cpu().double()                 # [K][H]
            where, ld = C.c_void_p(), C.c_int()
            P.check(L.mpc_ppo_update_layer_gradient(alg._handle, net, 0, C.byref(where), C.byref(ld)), "layer_gradient")
            assert ld.value == W0.shape[0]
            dY0 = _lib.device_view(where.value, (rows, ld.value), "<f4", torch.device(DEV)).cpu().double()
            exact, bound = dY0 @ W0, gamma(W0.shape[0] + 2) * (dY0.abs() @ W0.abs())
            err = (dy.double() - exact).abs()
            assert float(dY0.abs().max()) > 0 and dy.shape == (rows, H) and bool((err <= bound).all()), (net, float((err / bound).max()))
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"{_ids(case)}: d rows against float64 dY_0 W_0, largest error / bound {worst:.3f}")


def test_a_smaller_mini_batch_on_a_used_handle_equals_a_fresh_one():
    big, small = cases.SMALL[5], cases.SMALL[4]                                   # T = 5: 260 rows, then 85
    assert cases.case_rows(big) == 260 and cases.case_rows(small) == 85 and big[:3] == small[:3]
    dev, dst, used = _device(big, desired_kl=0.06)
    _grads_of(used, dst, 1)
    handle = used._handle.value
    _, small_dst, fresh = _device(small, desired_kl=0.06)
    used.cfg = fresh.cfg
    a = _grads_of(used, small_dst, 1)
    assert used._handle.value == handle and used._max_rows == 260 and used._seq_rows[0].shape == (85, 16)
    assert all(torch.equal(x, y) for x, y in zip(dev.parameters(), fresh.actor_critic.parameters()))      # (both fixtures draw the weights from one seed)
    b = _grads_of(fresh, small_dst, 1)
    assert fresh._max_rows == 85
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] and all(torch.equal(x, y) for x, y in zip(a[4], b[4]))


def test_state_refusals_come_before_any_launch():
    case = cases.SMALL[1]
    dev, dst, alg = _device(case)
    alg._device_state(cases.case_rows(case))                                     # a handle with the MLPs' tensors bound and nothing else
    L, err, p = P.update_lib(), P.update_lib().mpc_ppo_last_error, alg.lr_device.data_ptr()
    assert L.mpc_ppo_update_grads_sequence(alg._handle, 5, p, 0.2, 1.0, 0.01, 1, 0, 0.0, None, p, None) == -1 and b"no storage set" in err()
    flat = [getattr(dst, f).data_ptr() for f in ref.FIELDS]
    P.check(L.mpc_ppo_update_set_storage(alg._handle, dst.n * dst.T, *flat), "set_storage")
    assert L.mpc_ppo_update_grads_sequence(alg._handle, 5, p, 0.2, 1.0, 0.01, 1, 0, 0.0, None, p, None) == -1 and b"no dense rows set (mpc_ppo_update_set_sequence_rows)" in err()
    buf = torch.zeros(4 * 17 * 16 + 8, device=DEV)
    a = buf.data_ptr()
    step = 17 * 16 * 4
    assert L.mpc_ppo_update_set_sequence_rows(alg._handle, a, a + step, a + 2 * step, a + 3 * step - 16) == -1 and b"must not overlap" in err()
    assert L.mpc_ppo_update_set_sequence_rows(alg._handle, a, a + step, a + 2 * step, a + 3 * step) == 0
    assert L.mpc_ppo_update_set_sequence_rows(alg._handle, None, None, None, None) == 0
    assert L.mpc_ppo_update_grads_sequence(alg._handle, 5, p, 0.2, 1.0, 0.01, 1, 0, 0.0, None, p, None) == -1 and b"no dense rows set" in err()
    w = dev.memory_a.rnn.weight_ih_l0
    g = torch.zeros_like(w)
    one = lambda t: _lib.ptr_array([t.data_ptr()])
    assert L.mpc_ppo_update_bind_extra(alg._handle, 1, one(w), one(g), None, None, _lib.int_array([w.numel()])) == 0
    assert L.mpc_ppo_update_apply(alg._handle, 1.0, 0.9, 0.999, 1e-8, 1, p, None) == -1 and b"the extra tensors have no moments bound" in err()
    torch.cuda.synchronize()
    assert float(w.abs().max()) > 0 and not g.any()


def test_apply_without_extras_is_todays_apply_bit_for_bit():
    """``bind_extra(count=0)`` after extras were bound: the same norm partials, grids and tables as a handle that never saw the call."""
    torch.manual_seed(2)
    cpu = P.ActorCritic(16, 12, *cases.NETS, init_noise_std=0.7, num_critic_obs=16)
    grads = [torch.randn(p.shape) * 0.3 for p in cpu.bind_order()]
    out = []
    for extras in (False, True):
        dev = P.ActorCritic(16, 12, *cases.NETS, init_noise_std=0.7, num_critic_obs=16)
        dev.load_state_dict(cpu.state_dict())
        dev = dev.to(DEV)
        alg = P.PPO(dev, P.PPOConfig(actor_hidden_dims=cases.NETS[0], critic_hidden_dims=cases.NETS[1]), backend="hip")
        alg._device_state(8)
        L = P.update_lib()
        if extras:
            w = torch.randn(8192 + 4, device=DEV)                                # longer than any MLP tensor: more norm blocks while it is bound
            w0 = w.clone()
            t = [torch.zeros_like(w) for _ in range(3)]
            one = lambda x: _lib.ptr_array([x.data_ptr()])
            P.check(L.mpc_ppo_update_bind_extra(alg._handle, 1, one(w), one(t[0]), one(t[1]), one(t[2]), _lib.int_array([w.numel()])), "bind_extra")
            P.check(L.mpc_ppo_update_bind_extra(alg._handle, 0, None, None, None, None, None), "bind_extra")
        for s in range(2):
            for p, g in zip(dev.bind_order(), grads):
                p.grad.copy_(g * (s + 1))
            P.check(L.mpc_ppo_update_apply(alg._handle, 0.5, 0.9, 0.999, 1e-8, s + 1, alg.lr_device.data_ptr(), None), "apply")
        torch.cuda.synchronize()
        out.append([x.detach().cpu().clone() for p in dev.bind_order() for x in (p, p.grad, alg.optimizer.state[p]["exp_avg"], alg.optimizer.state[p]["exp_avg_sq"])])
        if extras:
            assert torch.equal(w, w0) and not any(x.any() for x in t)      # cleared: apply touched none of it
    assert all(torch.equal(a, b) for a, b in zip(*out))


# ---- 3. the whole update against float64 -------------------------------------------------------------------------------------------------------------------------
GAP_CASES = [cases.SMALL[4], cases.PRIVILEGED, cases.WIDE_STATE]


@pytest.mark.parametrize("case", GAP_CASES, ids=_ids)
def test_gradients_terms_and_decision_against_float64(case):
    I, H, nets, T, N, mb, wp = case
    cpu, st = _fixture(case)
    dev, dst, alg = _device(case, desired_kl=0.06)
    rel = lambda x, r: abs(x - r) / abs(r)
    sides = [(uref.grads_restated(cpu, alg.cfg, st, i), uref.grads_autograd(cpu, alg.cfg, st, i, torch.float32)) for i in range(mb)]
    pool3 = max(rel(t32[q], r64[1][q]) for r64, (_, t32) in sides for q in range(3))      # the three terms share a gap, the kl stands alone (tests/test_ppo_update.py)
    pool_kl = max(rel(t32[3], r64[1][3]) for r64, (_, t32) in sides)
    small = _small_gap([(r64[0], g32) for r64, (g32, _) in sides])
    for i in range(mb):
        (g64, t64, _, _), (g32, t32) = sides[i]
        for desired in (0.01, 0.06, 1.0):
            alg.cfg.desired_kl = desired
            _, got, terms, lr, _ = _grads_of(alg, dst, i)
            lo, hi = desired / 2.0, desired * 2.0
            assert min(abs(t64[3] - lo), abs(t64[3] - hi)) > abs(t32[3] - t64[3]), "the float64 kl is within gap of a threshold: the case decides nothing"
            assert lr == ref.adapt(1e-3, t64[3], alg.cfg), (desired, t64[3], lr)
        assert sorted(got) == sorted(g64) == sorted(g32) and len(got) == 2 * (len(nets[0]) + len(nets[1]) + 2) + 1 + 8
        for k in sorted(got):
            _gap_rule(got[k], g32[k], g64[k], f"{_ids(case)} mini-batch {i}: .grad of {k}", "gradients", small)
        for q, name in enumerate(("surrogate", "value loss", "entropy", "kl")):
            gap = pool_kl if q == 3 else pool3
            err = rel(float(terms[q]), t32[q])
            print(f"{_ids(case)} mini-batch {i}: {name} off torch's float32 by {err:.3e} (gap {gap:.3e}, ratio {err / gap:.3f})")
            RATIOS["terms"] = max(RATIOS.get("terms", 0.0), err / gap)
            assert gap > 0 and err <= 4 * gap, (name, err, gap)
    print("largest error / gap so far:", RATIOS)


@pytest.mark.parametrize("max_norm", (0.05, 1e3), ids=("clip", "no-clip"))
@pytest.mark.parametrize("steps", (1, 3))
def test_update_against_float64_adam(steps, max_norm):
    """``PPO.update`` with ``steps`` Adam steps (epochs of one mini-batch), the clip active and inactive: the learning-rate sequence is the float64 one;
    the parameter changes and both moments of all 19 tensors within 4 x the largest float32 gap of their kind, as tests/test_ppo_update_gpu.py holds them."""
    case = (48, 16, cases.NETS, 5, 17, 1, None)
    cpu, st = _fixture(case)
    kw = dict(desired_kl=0.01, num_learning_epochs=steps, max_grad_norm=max_norm)
    r64, r32 = (uref.update(cpu, _cfg(case, **kw), st, dt) for dt in (torch.float64, torch.float32))
    assert r64[1] == r32[1] and len(r64[1]) == steps and r64[1][0] != 1e-3
    dev, dst, alg = _device(case, **kw)
    alg.record_lr = True
    value_loss, surrogate = alg.update(dst)
    torch.cuda.synchronize()
    assert alg.lr_trace.tolist() == r64[1] and float(alg.lr_device) == r64[1][-1] and dst.step == 0
    named = dict(dev.named_parameters())
    assert len(named) == 19 and all(int(alg.optimizer.state[p]["step"]) == steps and not alg.optimizer.state[p]["step"].is_cuda for p in named.values())
    p0 = {k: v.detach().double() for k, v in cpu.named_parameters()}
    state = ({k: p.detach().cpu() for k, p in named.items()}, {k: alg.optimizer.state[p]["exp_avg"].cpu() for k, p in named.items()},
             {k: alg.optimizer.state[p]["exp_avg_sq"].cpu() for k, p in named.items()})
    for kind, what in enumerate(("parameter change", "exp_avg", "exp_avg_sq")):
        a64, a32 = (r64[0], r64[3], r64[4])[kind], (r32[0], r32[3], r32[4])[kind]
        off = lambda k: p0[k] if kind == 0 else 0.0
        gap = max(ref.rel_l2(a32[k].double() - off(k), a64[k] - off(k)) for k in named)
        errs = [(k, ref.rel_l2(state[kind][k].double() - off(k), a64[k] - off(k))) for k in named]
        worst = max(errs, key=lambda x: x[1])
        print(f"{steps} steps, max_norm {max_norm}: {what} largest error {worst[1]:.3e} ({worst[0]}), largest gap {gap:.3e}, ratio {worst[1] / gap:.3f}")
        RATIOS[what] = max(RATIOS.get(what, 0.0), worst[1] / gap)
        assert gap > 0 and all(e <= 4 * gap for _, e in errs), (what, worst, gap)
    norm = float(torch.cat([g.flatten() for g in uref.grads_autograd(cpu, _cfg(case, **kw), st, 0, torch.float64)[0].values()]).norm())
    assert (norm > max_norm) == (max_norm == 0.05), norm
    print("largest error / gap so far:", RATIOS)


def test_update_rerun_is_bit_identical_and_never_waits():
    case = cases.PRIVILEGED
    runs = []
    for _ in range(2):
        dev, dst, alg = _device(case, num_learning_epochs=2)
        alg.update(dst)                                                          # (the first update creates the handles and the optimiser state)
        dst.step = dst.T
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                                  # a torch call that waits for the device or copies to the host raises from here on
        try:
            out = alg.update(dst)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        runs.append([p.detach().cpu().clone() for p in dev.parameters()] + [alg.optimizer.state[p][k].cpu().clone() for p in dev.parameters() for k in ("exp_avg", "exp_avg_sq")]
                    + [out[0].cpu(), out[1].cpu(), alg.lr_device.cpu().clone()])
        assert all(int(alg.optimizer.state[p]["step"]) == 8 for p in dev.parameters())
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_adam_restrictions_are_refused():
    cpu, dev = uref.recurrent_pair(48, 16, cases.NETS, seed=1, update_through_time="hip", update_heads="hip")
    alg = P.PPO(dev.to(DEV))
    assert alg.device_update and alg.backend == "torch" and alg.lr_device.dtype == torch.float64
    for key, value in (("amsgrad", True), ("weight_decay", 0.1), ("maximize", True)):
        real = torch.optim.Adam

        def adam(params, lr, real=real, key=key, value=value):
            return real(params, lr=lr, **{key: value})
        torch.optim.Adam = adam
        try:
            with pytest.raises(ValueError, match="plain Adam"):
                P.PPO(dev)
        finally:
            torch.optim.Adam = real
    alg.set_learning_rate(3e-4)
    assert float(alg.lr_device) == 3e-4 and alg.optimizer.param_groups[0]["lr"] == 3e-4
    alg.lr_device.fill_(2e-4)
    alg.sync_learning_rate()
    assert alg.learning_rate == 2e-4 and alg.optimizer.param_groups[0]["lr"] == 2e-4


# ---- 4. the trainer ------------------------------------------------------------------------------------------------------------------------------------------------
N_ENVS, T_STEPS, H_TRAIN, TROT = 32, 4, 32, 0


def _pcfg():
    return P.PPOConfig(num_steps_per_env=T_STEPS, num_mini_batches=2, num_learning_epochs=1, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,), init_noise_std=0.5)


def _task(privileged=False):
    return R.BatchedRLTask([i % 3 for i in range(N_ENVS)], [TROT] * N_ENVS, cfg=R.TaskConfig(episode_length_s=0.03, seed=5), device=DEV,      # 3-tick episodes
                           privileged_obs=V.PrivilegedObs(N_ENVS, device=DEV) if privileged else None)


@pytest.fixture(scope="module")
def task():
    return _task()


def _config(heads):
    return RC.RecurrentConfig(hidden_size=H_TRAIN, update_through_time="hip", update_heads=heads)


def test_trainer_gradients_hip_heads_against_torch_heads(task):
    hip = P.PPOTrainer(task, _pcfg(), seed=11, recurrent=_config("hip"))
    other = P.PPOTrainer(task, _pcfg(), seed=11, recurrent=_config("torch"))
    other.actor_critic.load_state_dict(hip.actor_critic.state_dict())
    assert hip.alg.device_update and not other.alg.device_update and hip.actor_critic.update_heads == "hip"
    hip.collect()
    st = hip.storage
    assert st.dones.any() and not st.dones.all()
    _, g_hip, _, _, _ = _grads_of(hip.alg, st, 0)
    surrogate, value_loss, entropy, _ = other.alg.losses(next(st.recurrent_sequence_generator(2, 1)))
    other.actor_critic.zero_grad()
    (surrogate + other.alg.cfg.value_loss_coef * value_loss - other.alg.cfg.entropy_coef * entropy).backward()
    g_torch = {k: p.grad.detach().clone() for k, p in other.actor_critic.named_parameters()}
    cpu = uref.clone(hip.actor_critic, torch.float32)
    g64, _, _, _ = uref.grads_restated(cpu, _pcfg(), uref.storage_as(st, torch.float32), 0)
    g32, _ = uref.grads_autograd(cpu, _pcfg(), uref.storage_as(st, torch.float32), 0, torch.float32)
    assert sorted(g_hip) == sorted(g_torch) == sorted(g64) and len(g_hip) == 19
    small = _small_gap([(g64, g32)])
    for k in sorted(g_hip):
        _gap_rule(g_hip[k], g32[k], g64[k], f"trainer .grad of {k}", "trainer gradients", small)
        _gap_rule(g_torch[k], g32[k], g64[k], f"torch-heads trainer .grad of {k}", None, small)
    print("largest error / gap so far:", RATIOS)


def test_trainer_learns_and_checkpoints_move_between_the_settings(task, tmp_path):
    trainer = P.PPOTrainer(task, _pcfg(), seed=11, recurrent=_config("hip"))
    ac = trainer.actor_critic
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    trainer.learn(1)                                                             # (the first iteration creates the handles and the optimiser state)
    torch.cuda.synchronize()
    reads = []
    real = P._read_riders
    P._read_riders = lambda riders: reads.append(1) or real(riders)
    try:
        infos = trainer.learn(1)
    finally:
        P._read_riders = real
    assert len(reads) == 1 and len(infos) == 2 and all(np.isfinite(v) for info in infos for v in info.values() if isinstance(v, float))
    assert len(before) == 19 and all(not torch.equal(ac.state_dict()[k], v) for k, v in before.items()), [k for k, v in before.items() if torch.equal(ac.state_dict()[k], v)]
    assert infos[-1]["learning_rate"] == trainer.alg.learning_rate == float(trainer.alg.lr_device) == trainer.alg.optimizer.param_groups[0]["lr"]
    assert ac._seq.token == 4 and all(int(trainer.alg.optimizer.state[p]["step"]) == 4 for p in ac.parameters())
    path, back, plain = str(tmp_path / "hip.pt"), str(tmp_path / "torch.pt"), str(tmp_path / "plain.pt")
    trainer.save(path)
    ck = torch.load(path)
    other = P.PPOTrainer(task, _pcfg(), seed=4, recurrent=_config("torch"))
    other.save(plain)
    ck_plain = torch.load(plain)
    assert sorted(ck) == sorted(ck_plain) and sorted(ck["model_state_dict"]) == sorted(ck_plain["model_state_dict"])
    assert sorted(ck["optimizer_state_dict"]) == sorted(ck_plain["optimizer_state_dict"])
    assert ck["optimizer_state_dict"]["param_groups"][0]["params"] == ck_plain["optimizer_state_dict"]["param_groups"][0]["params"]
    assert sorted(ck["optimizer_state_dict"]["state"]) == list(range(19))
    probe = torch.randn(50, task.num_obs, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    ac.reset_memory()
    want = [ac.act_inference(probe).clone() for _ in range(2)]
    other.load(path)
    other.actor_critic.reset_memory()
    assert other.iteration == 2 and all(torch.equal(other.actor_critic.act_inference(probe), w) for w in want)
    assert np.isfinite(other.learn(1)[0]["value_loss"])                          # and trains on from it with torch's heads
    other.save(back)
    again = P.PPOTrainer(task, _pcfg(), seed=9, recurrent=_config("hip"))
    again.load(back)
    assert float(again.alg.lr_device) == other.alg.optimizer.param_groups[0]["lr"] == again.alg.learning_rate      # the device's rate follows the checkpoint's
    other.actor_critic.reset_memory(); again.actor_critic.reset_memory()
    assert again.iteration == 3 and torch.equal(again.actor_critic.act_inference(probe), other.actor_critic.act_inference(probe))
    info = again.learn(1)[0]
    assert np.isfinite(info["value_loss"]) and all(int(again.alg.optimizer.state[p]["step"]) == 8 for p in again.actor_critic.parameters())


def test_trainer_with_privileged_rows_and_normalisation():
    task = _task(privileged=True)
    trainer = P.PPOTrainer(task, _pcfg(), seed=3, normalize_obs=True, recurrent=_config("hip"))
    ac = trainer.actor_critic
    assert ac.memory_c.rnn.input_size == task.num_privileged_obs and ac.update_heads == "hip"
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    info = trainer.learn(1)[0]
    assert all(np.isfinite(info[k]) for k in ("mean_reward", "value_loss", "surrogate_loss", "mean_noise_std", "learning_rate"))
    assert all(not torch.equal(ac.state_dict()[k], v) for k, v in before.items()) and ac._seq.token == 2
