"""The recurrent actor-critic's update through time (csrc/mpc_recurrent_bptt.h, csrc/recurrent_bptt.h, ``RecurrentConfig(update_through_time=)``) without
a GPU: the float64 restatement of the backward pass (tests/recurrent_bptt_ref.py) against autograd, the dense roll against the padded trajectories --
the claim the design rests on --, the dense generator, every refusal of the C ABI and of the Python classes, and the kernels' resources in the
cross-compile."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, ppo as P, recurrent as RC, weight_policy as WP
from tests import recurrent_bptt_ref as bref, recurrent_ref as ref
from tests.helpers import ROOT
from tests.test_recurrent import H, I, N, PATTERNS, T, WP as WC, _model, _rolled

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
E_ARG = -1
SHAPES = ((1, 3, 16, 16), (5, 4, 48, 16), (6, 5, 64, 32))


def _case(T_, B, I_, H_, seed):
    g = torch.Generator().manual_seed(seed)
    mem = torch.nn.LSTM(I_, H_, 1)
    with torch.no_grad():
        for p in mem.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if p.dim() == 1 else 0.3))
    params = [mem.weight_ih_l0, mem.weight_hh_l0, mem.bias_ih_l0, mem.bias_hh_l0]
    xs, dY = torch.randn(T_, B, I_, generator=g), torch.randn(T_, B, H_, generator=g)
    h0, c0 = torch.rand(B, H_, generator=g) * 2 - 1, torch.rand(B, H_, generator=g) * 2 - 1
    return params, xs, h0, c0, dY


# ---- the restatement against autograd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_equals_float64_autograd(shape, pattern):
    T_, B, I_, H_ = shape
    params, xs, h0, c0, dY = _case(T_, B, I_, H_, seed=T_ + B)
    reset = bref.resets_from_dones(PATTERNS[pattern], T_, B)
    assert not reset[0].any() and (T_ == 1 or pattern in ("none",) or reset.any())
    got = bref.grads(xs, reset, h0, c0, params, dY)
    want = bref.autograd_grads(xs, reset, h0, c0, params, dY, torch.float64)
    for k in ("y", "c_last", "dW_ih", "dW_hh", "db"):
        assert float((got[k] - want[k]).abs().max()) <= 1e-10, k
    for t in range(T_):
        assert float((got["dG"][t] - want["dG"][t]).abs().max()) <= 1e-10, f"dG[{t}]"
    # the forward half is recurrent_ref.roll
    rh, rc, sh, sc = ref.roll(xs, reset, h0, c0, params)
    fwd = bref.forward(xs, reset, h0, c0, params)
    assert torch.equal(fwd["h_new"], rh) and torch.equal(fwd["c_new"], rc) and torch.equal(fwd["h_used"], sh) and torch.equal(fwd["c_used"], sc)


def test_forward_sequence_on_the_cpu_is_the_roll_and_differentiable():
    T_, B, I_, H_ = SHAPES[2]
    params, xs, h0, c0, dY = _case(T_, B, I_, H_, seed=2)
    mem = RC.Memory(I_, H_).double()
    with torch.no_grad():
        for p, q in zip(mem.parameters_in_bind_order(), params):
            p.copy_(q)
    reset = bref.resets_from_dones(PATTERNS["mixed"], T_, B)
    y = mem.forward_sequence(xs.double(), h0.double(), c0.double(), reset)
    want = bref.grads(xs, reset, h0, c0, params, dY)
    assert y.shape == (T_, B, H_) and float((y.detach() - want["y"]).abs().max()) <= 1e-12
    (y * dY.double()).sum().backward()
    for p, k in zip(mem.parameters_in_bind_order(), ("dW_ih", "dW_hh", "db", "db")):
        assert float((p.grad - want[k]).abs().max()) <= 1e-10, k
    plain = mem.forward_sequence(xs.double(), h0.double(), c0.double())           # no flags: zeros
    assert torch.equal(plain, mem.forward_sequence(xs.double(), h0.double(), c0.double(), torch.zeros(T_, B, dtype=torch.long)))


# ---- the dense path against the padded path -------------------------------------------------------------------------------------------------------------
def _loss_grads(ac, batch):
    alg = P.PPO(ac, P.PPOConfig())
    surrogate, value_loss, entropy, _ = alg.losses(batch)
    ac.zero_grad()
    (surrogate + alg.cfg.value_loss_coef * value_loss - alg.cfg.entropy_coef * entropy).backward()
    return {k: p.grad.clone() for k, p in ac.named_parameters()}


@pytest.mark.parametrize("privileged", (False, True))
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_dense_roll_equals_the_padded_trajectories(pattern, privileged):
    dones = PATTERNS[pattern]
    ac = _model(privileged)
    st, _, _ = _rolled(ac, dones, privileged)
    for x in (st.saved_h_a, st.saved_c_a, st.saved_h_c, st.saved_c_c):            # the premise: zero after each done
        assert not x[1:][dones[:-1, :, 0] != 0].any()
    for num_mini_batches in (1, 2, 5):
        padded = list(st.recurrent_mini_batch_generator(num_mini_batches, 1))
        dense = list(st.recurrent_sequence_generator(num_mini_batches, 1))
        assert len(padded) == len(dense) == num_mini_batches
        for p, d in zip(padded, dense):
            with torch.no_grad():
                want = ac.log_prob_entropy_value(p.obs, p.actions, p.critic_obs, masks=p.masks, hidden_states=(p.hidden_a, p.hidden_c))
                got = ac.log_prob_entropy_value(d.obs, d.actions, d.critic_obs, hidden_states=(d.hidden_a, d.hidden_c), reset=d.reset)
            for a, b, name in zip(got, want, ("log-prob", "entropy", "value", "mu", "sigma")):
                assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12, name
            g_padded, g_dense = _loss_grads(ac, p), _loss_grads(ac, d)
            assert sum(k.startswith("memory_") for k in g_dense) == 8
            for k in g_padded:
                assert float((g_dense[k] - g_padded[k]).abs().max()) <= 1e-10, k
    with pytest.raises(ValueError, match="not both"):
        ac.log_prob_entropy_value(d.obs, d.actions, d.critic_obs, masks=p.masks, hidden_states=(d.hidden_a, d.hidden_c), reset=d.reset)


# ---- the generator ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("privileged", (False, True))
def test_sequence_generator_yields_views_of_the_same_blocks(privileged):
    dones = PATTERNS["mixed"]
    st, _, _ = _rolled(_model(privileged), dones, privileged)
    want_reset = torch.cat((torch.zeros(1, N, dtype=torch.long), (dones[:-1, :, 0] != 0).long()))
    batches = list(st.recurrent_sequence_generator(2, 2))
    padded = list(st.recurrent_mini_batch_generator(2, 2))
    assert len(batches) == 4
    for k, (b, p) in enumerate(zip(batches, padded)):
        e0, e1 = (0, 2) if k % 2 == 0 else (2, 4)
        assert isinstance(b, RC.RecurrentSequenceBatch) and b._fields == tuple("reset" if f == "masks" else f for f in p._fields)
        # views, not copies: the storage's memory and strides
        assert b.obs.data_ptr() == st.observations[0, e0].data_ptr() and b.obs.shape == (T, 2, I) and b.obs.stride() == (N * I, I, 1)
        if privileged:
            assert b.critic_obs.data_ptr() == st.privileged_observations[0, e0].data_ptr() and b.critic_obs.stride() == (N * WC, WC, 1)
        else:
            assert b.critic_obs is None
        assert b.reset.dtype == torch.long and b.reset.shape == (T, 2) and b.reset.is_contiguous()
        assert not b.reset[0].any() and torch.equal(b.reset, want_reset[:, e0:e1])
        for got, other, full in zip(b[3:10], p[3:10], (st.actions, st.values, st.advantages, st.returns, st.actions_log_prob, st.mu, st.sigma)):
            assert got.data_ptr() == full[0, e0].data_ptr() and torch.equal(got, other)
        for (h0, c0), (sh, sc) in ((b.hidden_a, (st.saved_h_a, st.saved_c_a)), (b.hidden_c, (st.saved_h_c, st.saved_c_c))):
            assert h0.data_ptr() == sh[0, e0].data_ptr() and c0.data_ptr() == sc[0, e0].data_ptr() and h0.shape == (2, H) and h0.is_contiguous()
    with pytest.raises(ValueError, match="fewer environments"):
        next(P.RolloutStorage(1, T, "cpu", num_obs=I, hidden=(H, H)).recurrent_sequence_generator(2, 1))
    with pytest.raises(ValueError, match="hidden"):
        next(P.RolloutStorage(4, T, "cpu", num_obs=I).recurrent_sequence_generator(2, 1))


def test_update_picks_the_generator_by_the_option(monkeypatch):
    ac = _model(False)
    st, _, _ = _rolled(ac, PATTERNS["mixed"], False)
    called = []
    for name in ("recurrent_mini_batch_generator", "recurrent_sequence_generator"):
        real = getattr(st, name)
        monkeypatch.setattr(st, name, lambda *a, _n=name, _r=real: (called.append(_n), _r(*a))[1])
    alg = P.PPO(ac, P.PPOConfig(num_mini_batches=2, num_learning_epochs=1))
    alg.update(st)
    assert called == ["recurrent_mini_batch_generator"]                          # the default: today's path
    ac.update_through_time = "hip"                                               # float64 CPU tensors: the device path refuses them
    with pytest.raises(_lib.MpcLibraryError):
        alg.update(st)
    assert called[1:] == ["recurrent_sequence_generator"]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def _ints(*v):
    return C.cast((C.c_int * len(v))(*v), C.c_void_p)


def _ptrs(*v):
    return C.cast((C.c_void_p * len(v))(*v), C.c_void_p)


def test_abi_symbols_and_refusals_without_a_gpu():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "mpc_recurrent_bptt.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mpc_recurrent_bptt_[a-z_]+)\s*\(", header)))
    assert names == sorted(RC.BPTT_SYMBOLS) and len(names) == 9
    assert not set(RC.BPTT_SYMBOLS) & (set(_lib.SYMBOLS) | set(RC.SYMBOLS) | set(P.SYMBOLS) | set(WP.RECURRENT_SYMBOLS))
    L = RC.bptt_lib()
    err = L.mpc_recurrent_bptt_last_error
    h = C.c_void_p()

    def create(out=C.byref(h), memories=2, I_=_ints(48, 64), H_=_ints(32, 32), steps=6, rows=40):
        rc = L.mpc_recurrent_bptt_create(out, memories, I_, H_, steps, rows)
        assert rc == 0 or not h.value
        return rc
    for null in ("out", "I_", "H_"):
        assert create(**{null: None}) == E_ARG and b"null argument" in err(), null
    for bad in (0, 3):
        assert create(memories=bad) == E_ARG and b"one or two memories" in err()
    for bad in (0, -16, 40):
        assert create(I_=_ints(48, bad)) == E_ARG and f"memory 1: the input size {bad} is not a positive multiple of 16".encode() in err()
        assert create(H_=_ints(bad, 32)) == E_ARG and f"memory 0: the hidden size {bad} is not a positive multiple of 16".encode() in err()
    for bad in (0, -1):
        assert create(steps=bad) == E_ARG and b"max_steps must be at least 1" in err()
        assert create(rows=bad) == E_ARG and b"max_rows must be at least 1" in err()
    # LDS: the forward pass's 32 (I + H + 8) floats, the backward pass's 16 (4 H + 4): H = 624 is the widest state, 640 is over 160 KB
    assert create(memories=1, I_=_ints(1024), H_=_ints(256)) == E_ARG and b"forward pass" in err() and b"164864 bytes of LDS" in err()
    assert create(memories=1, I_=_ints(16), H_=_ints(640)) == E_ARG and b"backward pass" in err() and b"164096 bytes of LDS" in err()
    assert create(memories=1, I_=_ints(16), H_=_ints(256), steps=1 << 12, rows=1 << 12) == E_ARG and b"2^31" in err()
    assert L.mpc_recurrent_bptt_workspace_bytes(None) == -1
    assert create(memories=1, I_=_ints(16), H_=_ints(624)) == 0 and h.value      # a handle is host memory until it is bound
    L.mpc_recurrent_bptt_destroy(h)
    h.value = None
    assert create() == 0 and h.value
    R, chunks = 6 * 40, 1
    per_memory = lambda I_, H_: 4 * (11 * H_ * R + 4 * H_ * 64 + chunks * (4 * H_ * I_ + 4 * H_ * H_ + 4 * H_)) + 8 * R
    assert L.mpc_recurrent_bptt_workspace_bytes(h) == per_memory(48, 32) + per_memory(64, 32) + 4 * R      # the header's formula

    good = _ptrs(0x10000, 0x20000)
    bind = L.mpc_recurrent_bptt_bind
    assert bind(None, good, good, good, good) == E_ARG and b"null argument" in err()
    assert bind(h, good, None, good, good) == E_ARG and b"null argument" in err()
    assert bind(h, good, _ptrs(0x10000, 0), good, good) == E_ARG and b"memory 1: null parameter" in err()
    assert bind(h, good, good, _ptrs(0x10004, 0x20000), good) == E_ARG and b"memory 0" in err() and b"16-byte aligned" in err()

    io = lambda *rows: C.cast((RC.SeqIo * len(rows))(*[RC.SeqIo(*r) for r in rows]), C.c_void_p)
    ok_a = (0x100000, 40 * 48, 0x200000, 0x300000, 0x400000, 0x500000)            # x, stride, h0, c0, y [T B H = 7680 floats], c_last
    ok_c = (0x600000, 40 * 64, 0x700000, 0x800000, 0x900000, 0xa00000)
    both = io(ok_a, ok_c)
    fwd = L.mpc_recurrent_bptt_forward
    assert fwd(None, 6, 40, 0, 2, both, None, None) == E_ARG and b"null argument" in err()
    assert fwd(h, 6, 40, 0, 2, None, None, None) == E_ARG and b"null argument" in err()
    for bad in (0, -2, 7):
        assert fwd(h, bad, 40, 0, 2, both, None, None) == E_ARG and f"T = {bad} is outside 1 .. 6".encode() in err()
    for bad in (0, -2, 41):
        assert fwd(h, 6, bad, 0, 2, both, None, None) == E_ARG and f"B = {bad} is outside 1 .. 40".encode() in err()
    assert fwd(h, 6, 40, 1, 2, both, None, None) == E_ARG and b"memories 1 .. 2" in err()
    assert fwd(h, 6, 40, 0, 0, both, None, None) == E_ARG and b"memories" in err()
    assert fwd(h, 6, 40, 0, 2, both, 0x70004, None) == E_ARG and b"d_reset must be 8-byte aligned" in err()
    for k in (0, 2, 3, 4):
        bad = list(ok_c); bad[k] = None
        assert fwd(h, 6, 40, 0, 2, io(ok_a, tuple(bad)), None, None) == E_ARG and b"memory 1" in err() and b"is null" in err(), k
    for k in (0, 2, 3, 4, 5):
        bad = list(ok_a); bad[k] += 8
        assert fwd(h, 6, 40, 0, 2, io(tuple(bad), ok_c), None, None) == E_ARG and b"memory 0" in err() and b"16-byte aligned" in err(), k
    for stride, I_ in ((32, 48), (50, 48)):                                      # below one row; not a multiple of 4
        bad = list(ok_a); bad[1] = stride
        assert fwd(h, 6, 40, 0, 2, io(tuple(bad), ok_c), None, None) == E_ARG and f"the x stride {stride} must be a multiple of 4 floats and at least {I_}".encode() in err()
    bad = list(ok_c); bad[1] = 48                                                # the critic's memory reads 64 wide
    assert fwd(h, 6, 40, 0, 2, io(ok_a, tuple(bad)), None, None) == E_ARG and b"memory 1: the x stride 48" in err()
    bad = list(ok_a); bad[5] = ok_a[4] + 4 * 7680 - 16                           # c_last inside y
    assert fwd(h, 6, 40, 0, 2, io(tuple(bad), ok_c), None, None) == E_ARG and b"must not overlap" in err()
    bad = list(ok_c); bad[4] = ok_a[4] + 16                                      # the critic's y inside the actor's
    assert fwd(h, 6, 40, 0, 2, io(ok_a, tuple(bad)), None, None) == E_ARG and b"must not overlap" in err()
    assert fwd(h, 6, 40, 0, 2, both, 0x70008, None) == E_ARG and b"no parameters bound" in err()      # every check passed: nothing is bound
    assert fwd(h, 1, 1, 1, 1, io(ok_c[:5] + (None,)), None, None) == E_ARG and b"no parameters bound" in err()      # c_last and d_reset are optional

    grads = lambda *rows: C.cast((RC.SeqGrads * len(rows))(*[RC.SeqGrads(*r) for r in rows]), C.c_void_p)
    g_a = (0x100000, 0x200000, 0x300000, 0x400000, 0x500000)                      # dy, dW_ih, dW_hh, db_ih, db_hh
    g_c = (0x600000, 0x700000, 0x800000, 0x900000, 0xa00000)
    bwd = L.mpc_recurrent_bptt_backward
    assert bwd(None, 6, 40, 0, 2, grads(g_a, g_c), None) == E_ARG and b"null argument" in err()
    assert bwd(h, 6, 40, 0, 2, None, None) == E_ARG and b"null argument" in err()
    assert bwd(h, 7, 40, 0, 2, grads(g_a, g_c), None) == E_ARG and b"T = 7 is outside" in err()
    assert bwd(h, 6, 41, 0, 2, grads(g_a, g_c), None) == E_ARG and b"B = 41 is outside" in err()
    assert bwd(h, 6, 40, 0, 3, grads(g_a, g_c), None) == E_ARG and b"memories 0 .. 2" in err()
    for k in range(5):
        bad = list(g_a); bad[k] = None
        assert bwd(h, 6, 40, 0, 2, grads(tuple(bad), g_c), None) == E_ARG and b"memory 0" in err() and b"is null" in err(), k
        bad = list(g_c); bad[k] += 4
        assert bwd(h, 6, 40, 0, 2, grads(g_a, tuple(bad)), None) == E_ARG and b"memory 1" in err() and b"16-byte aligned" in err(), k
    bad = list(g_a); bad[4] = g_a[3] + 4 * 128 - 16                              # db_hh inside db_ih
    assert bwd(h, 6, 40, 0, 2, grads(tuple(bad), g_c), None) == E_ARG and b"must not overlap" in err()
    bad = list(g_c); bad[1] = g_a[2]                                             # the critic's dW_ih is the actor's dW_hh
    assert bwd(h, 6, 40, 0, 2, grads(g_a, tuple(bad)), None) == E_ARG and b"must not overlap" in err()
    assert bwd(h, 6, 40, 0, 2, grads(g_a, g_c), None) == E_ARG and b"no forward call to go back through" in err()      # every check passed
    again = L.mpc_recurrent_bptt_weight_gradients                                # the same refusals under its own name
    assert again(h, 6, 41, 0, 2, grads(g_a, g_c), None) == E_ARG and b"mpc_recurrent_bptt_weight_gradients: B = 41 is outside" in err()
    assert again(h, 6, 40, 0, 2, grads(g_a, g_c), None) == E_ARG and b"no forward call to go back through" in err()
    where = C.c_void_p()
    dg = L.mpc_recurrent_bptt_dgates
    assert dg(None, 0, C.byref(where)) == E_ARG and b"null argument" in err()
    assert dg(h, 0, None) == E_ARG and b"null argument" in err()
    for bad in (-1, 2):
        assert dg(h, bad, C.byref(where)) == E_ARG and f"memory {bad} of a handle with 2".encode() in err()
    assert dg(h, 1, C.byref(where)) == E_ARG and b"no workspace before mpc_recurrent_bptt_bind" in err() and not where.value
    L.mpc_recurrent_bptt_destroy(h)
    L.mpc_recurrent_bptt_destroy(None)


def test_python_refusals(monkeypatch):
    for make in (lambda: RC.RecurrentConfig(update_through_time="cuda"), lambda: RC.Memory(I, H, update_through_time="device"),
                 lambda: RC.ActorCriticRecurrent(I, 12, (32,), (32,), rnn_hidden_size=H, update_through_time=None)):
        with pytest.raises(ValueError, match="update_through_time=.*'torch' or 'hip'"):
            make()
    assert RC.RecurrentConfig().update_through_time == "torch" and RC.Memory(I, H).update_through_time == "torch"
    assert RC.ActorCriticRecurrent(I, 12, (32,), (32,), rnn_hidden_size=H).update_through_time == "torch"
    # "hip" on CPU tensors: refused, with or without a GPU in the box; no fallback to the torch loop
    mem = RC.Memory(I, H, update_through_time="hip")
    x, z = torch.zeros(3, 4, I), torch.zeros(4, H)
    with pytest.raises(_lib.MpcLibraryError, match="update_through_time"):
        mem.forward_sequence(x, z, z, None)
    ac = RC.ActorCriticRecurrent(I, 12, (32,), (32,), rnn_hidden_size=H, update_through_time="hip")
    with pytest.raises(_lib.MpcLibraryError, match="update_through_time"):
        ac.log_prob_entropy_value(x, torch.zeros(3, 4, 12), hidden_states=((z, z), (z, z)), reset=torch.zeros(3, 4, dtype=torch.long))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.MpcLibraryError, match="needs a GPU"):
        mem.forward_sequence(x, z, z, None)
    # PPO(backend="hip") / PPOTrainer(update="hip") stay refused, and say what exists now
    with pytest.raises(ValueError, match="not built.*update_through_time"):
        P.PPO(ac, backend="hip")
    with pytest.raises(ValueError, match="not built.*update_through_time"):
        P.PPOTrainer(None, update="hip", recurrent=RC.RecurrentConfig(hidden_size=H, update_through_time="hip"))


# ---- the kernels' resources ------------------------------------------------------------------------------------------------------------------------------
def test_sequence_kernels_compile_for_gfx950_without_scratch(tmp_path):
    out = tmp_path / "mpc_recurrent_bptt.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "mpc_recurrent_bptt.hip"), "-o", str(out)], check=True, capture_output=True, text=True)
    found = re.findall(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)",
                       r.stderr, re.S)
    caps = {"seq_forward_kernel": 192, "seq_backward_kernel": 216, "transpose_kernel": 16, "column_sum_kernel": 16}      # reported: 174 + 16, 194 + 16, 6, 8
    for kernel, cap in caps.items():
        mine = [f for f in found if kernel in f[0]]
        assert len(mine) == 1, found
        sgprs, vgprs, agprs, scratch, static_lds = (int(v) for v in mine[0][1:])
        print(f"{kernel}: {sgprs} SGPRs, {vgprs} VGPRs, {agprs} AGPRs, {scratch} scratch bytes, {static_lds} bytes of static LDS")
        # all LDS is dynamic; the caps are what the compile reports rounded up to the allocation granule of 8 (both sequence kernels keep two waves per SIMD)
        assert scratch == 0 and static_lds == 0 and vgprs + agprs <= cap
