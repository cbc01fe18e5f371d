"""The recurrent actor-critic's update through time on the MI355X (csrc/mpc_recurrent_bptt.h, csrc/recurrent_bptt.h, ``update_through_time="hip"``): the
roll against T launches of the cell kernel bit for bit, the backward pass against torch's float32 autograd under the rule of
tests/test_recurrent_gpu.py's _check_gap (4 x torch's own float32-vs-float64 gap, the float64 side being tests/recurrent_bptt_ref.py) per output tensor,
the reset flags, reruns, the parameters read in place, the dense generator without a host read, and the trainer."""
import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import ppo as P, privileged_obs as V, recurrent as RC, rl_task as R
from tests import recurrent_bptt_ref as bref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TROT = 0
HIDDEN = ((32, 16), (16,))
SHAPES = ((48, 16), (64, 32), (48, 144), (256, 256))      # (48, 144): an uneven trip of the column blocks (9 over 4 waves) and of the K = 4H loop's quads
STEPS = (1, 2, 5)
ROWS = (1, 15, 16, 17, 33)
A, C = RC.ACTOR, RC.CRITIC
PAD = 16                                                    # sentinel rows around every output
SENTINEL = 12345.0


def _cases(I, H):
    return ((3, 17),) if (I, H) == (256, 256) else tuple((T, B) for T in STEPS for B in ROWS)


def _pair(I, H, seed, critic_width=None):
    """tests/test_recurrent_gpu.py's recipe, restated: the same random recurrent actor-critic on the CPU and on the device, torch's default scale,
    biases x 0.1."""
    torch.manual_seed(seed)
    cpu = RC.ActorCriticRecurrent(I, 12, *HIDDEN, init_noise_std=0.5, num_critic_obs=critic_width, rnn_hidden_size=H)
    with torch.no_grad():
        for name, p in cpu.named_parameters():
            if p.dim() == 1 and name != "std":
                p.copy_(torch.randn_like(p) * 0.1)
    dev = RC.ActorCriticRecurrent(I, 12, *HIDDEN, init_noise_std=0.5, num_critic_obs=critic_width, rnn_hidden_size=H, update_through_time="hip")
    dev.load_state_dict(cpu.state_dict())
    return cpu, dev.to(DEV)


def _guarded(*shape):
    """(buffer, view): a device tensor of ``shape`` with PAD sentinel rows before and after it."""
    width = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    buf = torch.full((2 * PAD * width + int(np.prod(shape)),), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[PAD * width:PAD * width + int(np.prod(shape))].view(*shape)


def _intact(buf, view):
    width = int(np.prod(view.shape[1:])) if view.dim() > 1 else 1
    return bool((buf[:PAD * width] == SENTINEL).all()) and bool((buf[-PAD * width:] == SENTINEL).all())


class Problem:
    """A block of B environments e0 .. e0 + B - 1 of storages [T][N][width] with N > B and e0 > 0, states, flags and upstream gradients, on the CPU."""

    def __init__(self, T, B, widths, H, seed, flags=True):
        g = torch.Generator().manual_seed(seed)
        Hs = tuple(H) if isinstance(H, (tuple, list)) else (H,) * len(widths)      # one state width, or one per memory
        self.T, self.B, self.H, self.e0, self.N = T, B, H, 3, B + 7
        self.storage = [torch.randn(T, self.N, w, generator=g) for w in widths]
        self.xs = [s[:, self.e0:self.e0 + B] for s in self.storage]
        self.h0 = [torch.rand(B, h, generator=g) * 2 - 1 for h in Hs]
        self.c0 = [torch.rand(B, h, generator=g) * 2 - 1 for h in Hs]
        self.dy = [torch.randn(T, B, h, generator=g) for h in Hs]
        self.reset = torch.zeros(T, B, dtype=torch.long)
        if flags:
            self.reset[1:] = (torch.rand(T - 1, B, generator=g) < 0.3).long() * 3      # any non-zero value is a reset
            if T > 2:
                self.reset[T - 2, [0, B - 1]] = 1
            if T > 3:
                self.reset[2:4, B // 2] = -1                                            # two in a row


class Run:
    """One forward and one backward call of ``kernel`` on a Problem, every output between sentinel rows."""

    def __init__(self, kernel, pb, which=(A, C), reset="own", backward=True):
        T, B = pb.T, pb.B
        mems = [kernel.memories[w] for w in which]
        self.d_storage = [s.to(DEV) for s in pb.storage]
        xs = [s[:, pb.e0:pb.e0 + B] for s in self.d_storage]
        reset = (pb.reset.to(DEV) if reset == "own" else reset)
        ks = range(len(which))
        self.guards = []
        outs = []
        for m in mems:
            y, c = _guarded(T, B, m.hidden_size), _guarded(B, m.hidden_size)
            self.guards += [y, c]
            outs.append((y[1], c[1]))
        ys, cl = kernel.forward(which, xs, [pb.h0[k].to(DEV) for k in ks], [pb.c0[k].to(DEV) for k in ks], reset, c_last=True, out=outs)
        self.y, self.c_last = ys, cl
        self.grads, self.dG = None, None
        if backward:
            gouts = []
            for m in mems:
                gs = [_guarded(*p.shape) for p in m.parameters_in_bind_order()]
                self.guards += gs
                gouts.append([g[1] for g in gs])
            self.grads = kernel.backward(which, T, B, [pb.dy[k].to(DEV) for k in ks], out=gouts)
            self.dG = [kernel.dgates(w, T, B).clone() for w in which]
        torch.cuda.synchronize()
        assert all(_intact(b, v) for b, v in self.guards), "a sentinel row was written"
        assert all(torch.equal(d.cpu(), s) for d, s in zip(self.d_storage, pb.storage)), "the storage was written"

    def tensors(self, k):
        """The backward pass's output tensors of memory k by name."""
        g = self.grads[k]
        return {"dW_ih": g[0], "dW_hh": g[1], "db_ih": g[2], "db_hh": g[3], "dG": self.dG[k]}


def _kernel(dev):
    if dev._seq is None:
        dev._seq = RC.SequenceKernel(dev.memories())
    return dev._seq


def _gap_rule(got, t32, t64, what, ratios=None):
    """§8.3.4's rule on one tensor: the kernel may be off torch's float32 by 4 x torch's own distance from float64."""
    g, a, b = (t.detach().double().cpu().reshape(-1) for t in (got, t32, t64))
    gap, d = float((a - b).abs().max()), float((g - a).abs().max())
    ratio = d / gap if gap > 0 else (0.0 if d == 0 else float("inf"))
    print(f"{what}: off torch's float32 by {d:.3e}, gap {gap:.3e}, ratio {ratio:.3f} (bound 4)")
    if ratios is not None:
        ratios.append(ratio)
    assert d <= 4 * gap, f"{what}: off by {d:.3e} > 4 x {gap:.3e}"


# ---- 1. forward, bit for bit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,H", SHAPES)
def test_forward_equals_consecutive_cell_steps_bit_for_bit(I, H):
    Wc = 64 if I == 48 else 48                                                  # the critic's memory reads rows of another width in the same launch
    _, dev = _pair(I, H, seed=I + H, critic_width=Wc)
    kernel = _kernel(dev)
    for T, B in _cases(I, H):
        pb = Problem(T, B, (I, Wc), H, seed=100 * T + B)
        pb.reset[0, 0] = 1                                                      # the kernels take a flag at t = 0 as any other
        run = Run(kernel, pb, backward=False)
        d_reset = pb.reset.to(DEV)
        for m, h, c in zip(dev.memories(), pb.h0, pb.c0):
            dh, dc, _ = m.state(B, torch.device(DEV))
            dh.copy_(h); dc.copy_(c)
        for t in range(T):
            outs = dev.cell_step({A: run.d_storage[0][t, pb.e0:pb.e0 + B].contiguous(), C: run.d_storage[1][t, pb.e0:pb.e0 + B].contiguous()}, d_reset[t])
            for k in (A, C):
                assert torch.equal(run.y[k][t], outs[k]), f"y[{t}], memory {k}, T={T} B={B}"
        for k, m in enumerate(dev.memories()):                                   # the final state
            assert torch.equal(run.y[k][T - 1], m.h) and torch.equal(run.c_last[k], m.c), f"final state, memory {k}, T={T} B={B}"


# ---- 2. backward, by the gap rule, per output tensor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,H", SHAPES)
def test_backward_against_float64_per_tensor(I, H):
    """Measured on the MI355X, the largest ratio over a shape's cases per tensor (dW_ih, dW_hh, db, dG): (48, 16) 3.11, 3.60, 3.87, 3.87; (64, 32) 2.40, 3.32,
    3.97, 3.53; (48, 144) 3.12, 2.89, 3.23, 3.26; (256, 256) 2.03, 2.15, 2.57, 2.50."""
    cpu, dev = _pair(I, H, seed=I + H + 1)
    kernel = _kernel(dev)
    worst = {}
    for T, B in _cases(I, H):
        pb = Problem(T, B, (I, I), H, seed=7 * T + B)
        run = Run(kernel, pb)
        for k, m in enumerate(cpu.memories()):
            params = m.parameters_in_bind_order()
            t64 = bref.grads(pb.xs[k], pb.reset, pb.h0[k], pb.c0[k], params, pb.dy[k])
            t32 = bref.autograd_grads(pb.xs[k], pb.reset, pb.h0[k], pb.c0[k], params, pb.dy[k], torch.float32)
            for name, got in run.tensors(k).items():
                key = "db" if name.startswith("db") else name
                ratios = worst.setdefault(name, [])
                _gap_rule(got, t32[key], t64[key], f"I={I} H={H} T={T} B={B} memory {k} {name}", ratios)
            assert torch.equal(run.grads[k][2], run.grads[k][3])                 # db_ih and db_hh are the same sums
    print({name: round(max(r), 3) for name, r in worst.items()})


def _check_memory(run, k, pb, j, params, what):
    """The gap rule on every output tensor of the run's memory k, which is the problem's memory j with the CPU parameters ``params``."""
    t64 = bref.grads(pb.xs[j], pb.reset, pb.h0[j], pb.c0[j], params, pb.dy[j])
    t32 = bref.autograd_grads(pb.xs[j], pb.reset, pb.h0[j], pb.c0[j], params, pb.dy[j], torch.float32)
    for name, got in run.tensors(k).items():
        _gap_rule(got, t32["db" if name.startswith("db") else name], t64["db" if name.startswith("db") else name], f"{what} {name}")


def _sub_problem(pb, j):
    """Memory j of a problem as a one-memory problem: the same rows, states, flags and upstream gradients."""
    one = Problem(pb.T, pb.B, (pb.storage[j].shape[2],), pb.h0[j].shape[1], seed=0, flags=False)
    one.storage, one.h0, one.c0, one.dy, one.reset = [pb.storage[j]], [pb.h0[j]], [pb.c0[j]], [pb.dy[j]], pb.reset
    one.xs = [pb.xs[j]]
    return one


def test_backward_with_memories_of_different_widths_and_one_memory_at_a_time():
    T, B = 5, 17
    # (I_a, I_c) = (48, 64) in one backward call
    cpu, dev = _pair(48, 32, seed=51, critic_width=64)
    kernel = _kernel(dev)
    pb = Problem(T, B, (48, 64), 32, seed=13)
    both = Run(kernel, pb)
    for k, m in enumerate(cpu.memories()):
        _check_memory(both, k, pb, k, m.parameters_in_bind_order(), f"I = (48, 64), memory {k}")
    # first = 1, count = 1: the critic's memory alone computes the bits it computes beside the actor's
    alone = Run(kernel, _sub_problem(pb, C), which=(C,))
    assert torch.equal(alone.y[0], both.y[C]) and torch.equal(alone.c_last[0], both.c_last[C])
    for name, t in alone.tensors(0).items():
        assert torch.equal(t, both.tensors(C)[name]), name
    # (I, H) = (48, 16) and (64, 32) in one call: a handle over two bare memories
    torch.manual_seed(52)
    mems = [RC.Memory(48, 16), RC.Memory(64, 32)]
    twins = [RC.Memory(48, 16).to(DEV), RC.Memory(64, 32).to(DEV)]
    for m, d in zip(mems, twins):
        d.load_state_dict(m.state_dict())
    pb2 = Problem(T, B, (48, 64), (16, 32), seed=14)
    mixed = Run(RC.SequenceKernel(twins), pb2)
    for k, m in enumerate(mems):
        _check_memory(mixed, k, pb2, k, m.parameters_in_bind_order(), f"H = (16, 32), memory {k}")
    # Memory.forward_sequence with the option: the one-memory autograd path
    torch.manual_seed(53)
    ref_mem = RC.Memory(48, 32)
    mem = RC.Memory(48, 32, update_through_time="hip").to(DEV)
    mem.load_state_dict(ref_mem.state_dict())
    pb3 = Problem(T, B, (48,), 32, seed=15)
    storage = pb3.storage[0].to(DEV)
    y = mem.forward_sequence(storage[:, pb3.e0:pb3.e0 + B], pb3.h0[0].to(DEV), pb3.c0[0].to(DEV), pb3.reset.to(DEV))
    (y * pb3.dy[0].to(DEV)).sum().backward()
    params = ref_mem.parameters_in_bind_order()
    t64 = bref.grads(pb3.xs[0], pb3.reset, pb3.h0[0], pb3.c0[0], params, pb3.dy[0])
    t32 = bref.autograd_grads(pb3.xs[0], pb3.reset, pb3.h0[0], pb3.c0[0], params, pb3.dy[0], torch.float32)
    for p, key in zip(mem.parameters_in_bind_order(), ("dW_ih", "dW_hh", "db", "db")):
        _gap_rule(p.grad, t32[key], t64[key], f"Memory.forward_sequence .grad {key}")


def test_rows_are_kept_alive_between_forward_and_backward():
    """The backward pass reads x in place: a temporary x must survive until then, and a write to it in between must be refused."""
    T, B, I, H = 5, 33, 64, 32
    torch.manual_seed(61)
    mem = RC.Memory(I, H, update_through_time="hip").to(DEV)
    pb = Problem(T, B, (I,), H, seed=16)
    rows, h0, c0, reset, dy = pb.xs[0].contiguous().to(DEV), pb.h0[0].to(DEV), pb.c0[0].to(DEV), pb.reset.to(DEV), pb.dy[0].to(DEV)

    def grads(hold):
        mem.zero_grad()
        x = rows * 1.0                                                          # a temporary: nothing but the autograd node refers to it after the call
        y = mem.forward_sequence(x, h0, c0, reset)
        if not hold:
            del x
        junk = [torch.full_like(rows, float("nan")) for _ in range(4)]          # what the caching allocator would hand a freed block to
        (y * dy).sum().backward()
        del junk
        return [p.grad.clone() for p in mem.parameters_in_bind_order()]
    held, dropped = grads(True), grads(False)
    assert all(torch.isfinite(g).all() for g in dropped) and all(torch.equal(a, b) for a, b in zip(held, dropped))
    x = rows * 1.0
    y = mem.forward_sequence(x, h0, c0, reset)
    x.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()


def test_backward_refuses_what_is_not_the_last_forward():
    from rl_mpc_locomotion_amd import _lib
    I, H, T, B = 48, 16, 3, 5
    _, dev = _pair(I, H, seed=71)
    kernel = _kernel(dev)
    pb = Problem(T, B, (I, I), H, seed=17)
    Run(kernel, pb, backward=False)
    dys = [d.to(DEV) for d in pb.dy]
    for args, text in (((2, B), "T = 2, B = 5"), ((T, 4), "T = 3, B = 4")):
        with pytest.raises(_lib.MpcLibraryError, match=f"{text}, memories 0 .. 1 do not match the last forward call's T = 3, B = 5, memories 0 .. 1"):
            kernel.backward((A, C), *args, [d[:args[0], :args[1]].contiguous() for d in dys])
    with pytest.raises(_lib.MpcLibraryError, match="memories 1 .. 1 do not match the last forward call's"):
        kernel.backward((C,), T, B, dys[1:])
    with pytest.raises(_lib.MpcLibraryError, match="no backward call since the last forward call"):
        kernel.backward((A, C), T, B, dys, entry="mpc_recurrent_bptt_weight_gradients")
    assert len(kernel.backward((A, C), T, B, dys)) == 2                          # the matching call goes through after the refusals
    # the autograd node of a roll whose workspace a later roll has overwritten
    storage = [s.to(DEV) for s in pb.storage]
    xs = [s[:, pb.e0:pb.e0 + B] for s in storage]
    state = [t.to(DEV) for t in pb.h0], [t.to(DEV) for t in pb.c0]
    first = RC.roll_on_device(kernel, (A, C), xs, *state, None)
    second = RC.roll_on_device(kernel, (A, C), xs, *state, None)
    with pytest.raises(RuntimeError, match="the workspace holds a later forward call"):
        first[0].sum().backward()
    second[0].sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in dev.memory_a.parameters_in_bind_order())


# ---- 3. flags -----------------------------------------------------------------------------------------------------------------------------------------
def test_flags_cut_the_carries_and_leave_other_rows_alone():
    I, H, T, B, cut = 48, 32, 5, 17, 3
    _, dev = _pair(I, H, seed=21)
    kernel = _kernel(dev)
    pb = Problem(T, B, (I, I), H, seed=5, flags=False)
    flagged = [0, 15, 16]
    pb.reset[cut, flagged] = 1
    full = Run(kernel, pb)
    # the two halves as calls of their own: slots 0 .. cut-1, and slots cut .. T-1 from a state the flag zeroes
    first, second = Problem(cut, B, (I, I), H, seed=5, flags=False), Problem(T - cut, B, (I, I), H, seed=5, flags=False)
    for k in range(2):
        first.storage[k], second.storage[k] = pb.storage[k][:cut].contiguous(), pb.storage[k][cut:].contiguous()
        first.h0[k], first.c0[k], first.dy[k], second.dy[k] = pb.h0[k], pb.c0[k], pb.dy[k][:cut].contiguous(), pb.dy[k][cut:].contiguous()
    second.reset[0, flagged] = 1
    for half in (first, second):
        half.N, half.xs = pb.N, None
    a, b = Run(kernel, first), Run(kernel, second)
    for k in range(2):
        assert torch.equal(full.dG[k][:cut, flagged], a.dG[k][:, flagged])       # nothing of slots cut .. reached slot cut - 1 on the flagged rows
        assert torch.equal(full.dG[k][cut:, flagged], b.dG[k][:, flagged]) and torch.equal(full.y[k][cut:, flagged], b.y[k][:, flagged])
        assert torch.equal(full.y[k][:cut], a.y[k])
    # reset all zero equals no resets; unflagged rows do not move with other rows' flags
    plain, zeros = Run(kernel, pb, reset=None), Run(kernel, pb, reset=torch.zeros(T, B, dtype=torch.long, device=DEV))
    others = [r for r in range(B) if r not in flagged]
    for k in range(2):
        assert torch.equal(plain.y[k], zeros.y[k]) and torch.equal(plain.dG[k], zeros.dG[k]) and torch.equal(plain.c_last[k], zeros.c_last[k])
        assert all(torch.equal(p, z) for p, z in zip(plain.grads[k], zeros.grads[k]))
        assert torch.equal(full.y[k][:, others], plain.y[k][:, others]) and torch.equal(full.dG[k][:, others], plain.dG[k][:, others])
        assert not torch.equal(full.dG[k][:cut, flagged], plain.dG[k][:cut, flagged]) and not torch.equal(full.y[k][cut:, flagged], plain.y[k][cut:, flagged])


# ---- 4. a rerun ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_rerun_is_bit_identical():
    I, H, T, B = 48, 144, 5, 33
    _, dev = _pair(I, H, seed=31)
    pb = Problem(T, B, (I, I), H, seed=9)
    one, two = Run(_kernel(dev), pb), Run(_kernel(dev), pb)
    for k in range(2):
        assert torch.equal(one.y[k], two.y[k]) and torch.equal(one.c_last[k], two.c_last[k])
        for name, t in one.tensors(k).items():
            assert torch.equal(t, two.tensors(k)[name]), name


# ---- 5. the parameters are read in place ----------------------------------------------------------------------------------------------------------------
def test_an_in_place_add_is_seen_by_the_next_call():
    I, H, T, B = 64, 32, 5, 17
    cpu, dev = _pair(I, H, seed=41)
    kernel = _kernel(dev)
    pb = Problem(T, B, (I, I), H, seed=11)
    before = Run(kernel, pb)
    with torch.no_grad():
        delta = torch.randn_like(cpu.memory_a.rnn.weight_hh_l0) * 0.2
        cpu.memory_a.rnn.weight_hh_l0.add_(delta)
        dev.memory_a.rnn.weight_hh_l0.add_(delta.to(DEV))                        # in place: the same address, no rebinding
    ptrs = kernel._ptrs
    after = Run(kernel, pb)
    assert kernel._ptrs == ptrs
    assert (after.y[A] - before.y[A]).abs().max() > 1e-2 and (after.dG[A] - before.dG[A]).abs().max() > 1e-3      # forward and W_hh^T both follow
    assert torch.equal(after.y[C], before.y[C]) and all(torch.equal(x, y) for x, y in zip(after.grads[C], before.grads[C]))      # (the critic's was not touched)
    fresh = Run(RC.SequenceKernel(dev.memories()), pb)                           # a handle bound after the change computes the same bits
    for name, t in after.tensors(A).items():
        assert torch.equal(t, fresh.tensors(A)[name]), name
    params = cpu.memory_a.parameters_in_bind_order()
    t64 = bref.grads(pb.xs[A], pb.reset, pb.h0[A], pb.c0[A], params, pb.dy[A])
    t32 = bref.autograd_grads(pb.xs[A], pb.reset, pb.h0[A], pb.c0[A], params, pb.dy[A], torch.float32)
    for name, got in after.tensors(A).items():
        key = "db" if name.startswith("db") else name
        _gap_rule(got, t32[key], t64[key], f"after an in-place add_: {name}")


# ---- 6. the generator makes no host read ------------------------------------------------------------------------------------------------------------------
def test_sequence_generator_runs_without_a_host_read():
    T, N, I, H = 5, 12, 48, 32
    st = P.RolloutStorage(N, T, DEV, num_obs=I, num_privileged_obs=64, hidden=(H, H))
    st.dones.copy_((torch.rand(T, N, 1, generator=torch.Generator().manual_seed(2)) < 0.3).float())
    want = torch.cat((torch.zeros(1, N, dtype=torch.long, device=DEV), (st.dones[:-1, :, 0] != 0).long()))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")          # a torch call that waits for the device or copies to the host raises from here on
    try:
        batches = list(st.recurrent_sequence_generator(3, 2))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(batches) == 6
    for k, b in enumerate(batches):
        e0 = 4 * (k % 3)
        assert b.obs.data_ptr() == st.observations[0, e0].data_ptr() and b.obs.stride() == (N * I, I, 1) and b.critic_obs.stride() == (N * 64, 64, 1)
        assert b.reset.is_contiguous() and torch.equal(b.reset, want[:, e0:e0 + 4]) and b.hidden_a[0].data_ptr() == st.saved_h_a[0, e0].data_ptr()


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------------------
N_ENVS, T_STEPS, H_TRAIN = 32, 4, 32


def _pcfg():
    return P.PPOConfig(num_steps_per_env=T_STEPS, num_mini_batches=2, num_learning_epochs=1, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,),
                       init_noise_std=0.5)


def _task(privileged=False):
    return R.BatchedRLTask([i % 3 for i in range(N_ENVS)], [TROT] * N_ENVS, cfg=R.TaskConfig(episode_length_s=0.03, seed=5), device=DEV,      # 3-tick episodes
                           privileged_obs=V.PrivilegedObs(N_ENVS, device=DEV) if privileged else None)


@pytest.fixture(scope="module")
def task():
    return _task()


def _config(through):
    return RC.RecurrentConfig(hidden_size=H_TRAIN, update_through_time=through)


def _first_batch_grads(alg, storage, generator):
    surrogate, value_loss, entropy, _ = alg.losses(next(getattr(storage, generator)(2, 1)))
    alg.actor_critic.zero_grad()
    (surrogate + alg.cfg.value_loss_coef * value_loss - alg.cfg.entropy_coef * entropy).backward()
    return {k: p.grad.detach().clone() for k, p in alg.actor_critic.named_parameters()}


# ---- 7. hip against torch on one collected storage ----------------------------------------------------------------------------------------------------------
def test_trainer_gradients_hip_against_torch(task):
    hip = P.PPOTrainer(task, _pcfg(), seed=11, recurrent=_config("hip"))
    ref_trainer = P.PPOTrainer(task, _pcfg(), seed=11, recurrent=_config("torch"))
    ref_trainer.actor_critic.load_state_dict(hip.actor_critic.state_dict())
    assert hip.actor_critic.update_through_time == "hip" and ref_trainer.actor_critic.update_through_time == "torch"
    hip.collect()
    st = hip.storage
    assert st.dones.any() and not st.dones.all()
    g_hip = _first_batch_grads(hip.alg, st, "recurrent_sequence_generator")
    g_torch = _first_batch_grads(ref_trainer.alg, st, "recurrent_mini_batch_generator")
    # float64: the same storage and parameters on the CPU, the dense roll through torch's loop
    cpu = RC.ActorCriticRecurrent(task.num_obs, 12, (64, 32), (32,), init_noise_std=0.5, rnn_hidden_size=H_TRAIN).double()
    cpu.load_state_dict({k: v.detach().cpu().double() for k, v in hip.actor_critic.state_dict().items()})
    st64 = P.RolloutStorage(N_ENVS, T_STEPS, "cpu", num_obs=task.num_obs, hidden=(H_TRAIN, H_TRAIN))
    for k, v in list(vars(st).items()):
        if torch.is_tensor(v):
            setattr(st64, k, v.detach().cpu().double())
    g64 = _first_batch_grads(P.PPO(cpu, _pcfg()), st64, "recurrent_sequence_generator")
    assert sorted(g_hip) == sorted(g_torch) == sorted(g64) and sum(k.startswith("memory_") for k in g_hip) == 8
    for k in sorted(g_hip):
        _gap_rule(g_hip[k], g_torch[k], g64[k], f"trainer .grad of {k}")


# ---- 8. the trainer end to end --------------------------------------------------------------------------------------------------------------------------------
def test_trainer_learns_with_the_device_roll_and_checkpoints_move_between_the_settings(task, tmp_path):
    trainer = P.PPOTrainer(task, _pcfg(), seed=11, recurrent=_config("hip"))
    ac = trainer.actor_critic
    before = {k: v.clone() for k, v in ac.state_dict().items() if k.startswith("memory_")}
    infos = trainer.learn(2)
    assert len(infos) == 2 and all(np.isfinite(v) for info in infos for v in info.values() if isinstance(v, float))
    assert len(before) == 8 and all(not torch.equal(ac.state_dict()[k], v) for k, v in before.items())
    assert ac._seq is not None and ac._seq.token == 4 and ac._seq.workspace_bytes() > 0                  # two iterations of two mini-batches went through the handle
    # a checkpoint of the "hip" trainer into a "torch" trainer and back: the same keys, the same policy
    path, back = str(tmp_path / "hip.pt"), str(tmp_path / "torch.pt")
    trainer.save(path)
    ck = torch.load(path)
    other = P.PPOTrainer(task, _pcfg(), seed=4, recurrent=_config("torch"))
    plain = str(tmp_path / "plain.pt")
    other.save(plain)
    ck_plain = torch.load(plain)
    assert sorted(ck) == sorted(ck_plain) and sorted(ck["model_state_dict"]) == sorted(ck_plain["model_state_dict"])
    assert sorted(ck["optimizer_state_dict"]) == sorted(ck_plain["optimizer_state_dict"])
    assert ck["optimizer_state_dict"]["param_groups"][0]["params"] == ck_plain["optimizer_state_dict"]["param_groups"][0]["params"]
    probe = torch.randn(50, task.num_obs, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    ac.reset_memory()
    want = [ac.act_inference(probe).clone() for _ in range(2)]
    other.load(path)
    other.actor_critic.reset_memory()
    assert other.iteration == 2 and all(torch.equal(other.actor_critic.act_inference(probe), w) for w in want)
    assert np.isfinite(other.learn(1)[0]["value_loss"])                          # and trains on from it with the torch update
    other.save(back)
    again = P.PPOTrainer(task, _pcfg(), seed=9, recurrent=_config("hip"))
    again.load(back)
    other.actor_critic.reset_memory(); again.actor_critic.reset_memory()
    assert again.iteration == 3 and torch.equal(again.actor_critic.act_inference(probe), other.actor_critic.act_inference(probe))
    assert np.isfinite(again.learn(1)[0]["value_loss"])


def test_trainer_with_privileged_rows_and_normalisation():
    task = _task(privileged=True)
    trainer = P.PPOTrainer(task, _pcfg(), seed=3, normalize_obs=True, recurrent=_config("hip"))
    ac = trainer.actor_critic
    assert ac.memory_c.rnn.input_size == task.num_privileged_obs and ac.update_through_time == "hip"
    before = {k: v.clone() for k, v in ac.state_dict().items() if k.startswith("memory_")}
    info = trainer.learn(1)[0]
    assert all(np.isfinite(info[k]) for k in ("mean_reward", "value_loss", "surrogate_loss", "mean_noise_std", "learning_rate"))
    assert all(not torch.equal(ac.state_dict()[k], v) for k, v in before.items()) and ac._seq.token == 2
