"""Teacher-student policy distillation on the MI355X: mpc_ac_act_distill against the two launches it stands for, bit for bit; the behaviour-cloning
update (mpc_ppo_update_grads_distill, mpc_ppo_update_apply_actor, Distillation(backend="hip")) against float64 autograd and Adam on the CPU
(tests/distill_ref.py); and the three stages end to end on a task with privileged observations.

The tolerance is the project's rule (tests/test_ppo_update_gpu.py): at most 4 x the distance of torch's own float32 run from the float64 run.  The
distance is pooled, because a single tensor's is one draw of a rounding error: gradients tensor by tensor in relative L2, each held to 4 x the largest
per-tensor gap over all row counts and both loss types of the same net; the two scalar terms share the largest of their relative gaps over the same
cases.  The 8192-row case has a pool of its own.  tests/test_distill.py pins which GEMM kernel each launch of these cases reaches.  Largest measured
ratios error / gap: DESIGN.md section 8.3.8."""
import ctypes as C

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, distill as D, ppo as P
from rl_mpc_locomotion_amd.weight_policy import WeightPolicy
from tests import distill_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TYPES = ("mse", "huber")
NETS = {"uneven": ((32, 16), (64,)), "odd": ((80, 48), (144,))}
ROWS = {"single": 1, "ragged": 97, "two heads": 257, "chunked": 1040}              # mini-batch rows
STORAGE = {"single": (1, 1), "ragged": (65, 6), "two heads": (65, 6), "chunked": (65, 16)}      # (n, T) they are drawn from: 1, 390 (permuted), 390, 1040 rows
BIG_NETS, BIG_ROWS, BIG_STORAGE, BIG_WIDTH = ((512, 256, 128), (512, 256, 128)), 8192, (1024, 8), 48


# ---- the collection launch
def _pair(student_width, teacher_width, seed=1):
    """(student, teacher) on the device: other depths, other widths; biases of size 0.1 and a std that differs from action to action."""
    torch.manual_seed(seed)
    student = P.ActorCritic(student_width, 12, (32, 16), (64,), num_critic_obs=teacher_width)
    teacher = P.ActorCritic(teacher_width, 12, (64,), (32,))
    with torch.no_grad():
        student.std.copy_(torch.rand(12) * 0.5 + 0.05)
        for net in (student, teacher):
            for p in net.parameters():
                if p.dim() == 1 and p is not net.std:
                    p.copy_(torch.randn_like(p) * 0.1)
    return student.to(DEV), teacher.to(DEV)


def _rows(n, w, seed):
    return (torch.randn((n, w), generator=torch.Generator().manual_seed(seed)) * 1.5).to(DEV)


@pytest.mark.parametrize("n", (37, 1))
@pytest.mark.parametrize("widths", ((48, 64), (240, 256)))
def test_act_distill_is_the_students_act_and_the_teachers_inference(widths, n):
    """37 rows are three 16-row tiles, the last with 5 live rows.  Every output is written into the head of a longer buffer whose tail must stay."""
    student, teacher = _pair(*widths)
    obs, tobs = _rows(n, widths[0], 3), _rows(n, widths[1], 4)
    teacher_before = [p.detach().clone() for p in teacher.parameters()]
    want = student.act(obs, seed=9, step=5, return_eps=True, critic_obs=tobs)
    label = teacher.act_inference(tobs)
    guard = {k: torch.full((n + 3, 12), 7.0, device=DEV) for k in ("actions", "mu", "sigma", "teacher_actions")}
    out = D.act_distill(student, teacher, obs, tobs, seed=9, step=5, out={k: v[:n] for k, v in guard.items()}, return_eps=True)
    for k in ("actions", "mu", "sigma", "eps"):
        assert torch.equal(out[k], want[k]), k
    assert torch.equal(out["teacher_actions"], label) and not torch.equal(label, want["mu"])
    assert all(bool((v[n:] == 7.0).all()) for v in guard.values())
    assert float(out["eps"].abs().max()) > 0 and torch.equal(out["actions"], want["mu"] + want["sigma"] * want["eps"])
    assert all(torch.equal(a, b) for a, b in zip(teacher_before, teacher.parameters()))
    # another step draws other noise under the same mean; fresh tensors when no slot is given
    other = D.act_distill(student, teacher, obs, tobs, seed=9, step=6)
    assert torch.equal(other["mu"], want["mu"]) and not torch.equal(other["actions"], want["actions"]) and torch.equal(other["teacher_actions"], label)
    # the existing launches keep their bits beside it: the student's value is the critic's of the privileged rows
    assert torch.equal(want["values"], student.evaluate(tobs))


def test_act_distill_refuses_before_the_launch():
    student, teacher = _pair(48, 64)
    obs, tobs = _rows(5, 48, 3), _rows(5, 64, 4)
    with pytest.raises(ValueError, match="obs must be"):
        D.act_distill(student, teacher, tobs, tobs, 1, 0)
    with pytest.raises(ValueError, match="obs must be"):
        D.act_distill(student, teacher, obs, obs, 1, 0)
    with pytest.raises(ValueError, match="different numbers of rows"):
        D.act_distill(student, teacher, obs, tobs[:4].contiguous(), 1, 0)
    with pytest.raises(ValueError, match="teacher_actions must be"):
        D.act_distill(student, teacher, obs, tobs, 1, 0, out={k: torch.zeros((5, 12 if k != "teacher_actions" else 1), device=DEV)
                                                              for k in ("actions", "mu", "sigma", "teacher_actions")})


# ---- the gradients
def _fixture(nets, rows):
    """(CPU student, CPU storage, the mini-batch's index) of one case: in-range indices only."""
    hidden = NETS[nets] if nets in NETS else BIG_NETS
    n, T = STORAGE[rows] if rows in STORAGE else BIG_STORAGE
    count = ROWS[rows] if rows in ROWS else BIG_ROWS
    ac, st = ref.fixture(hidden, n, T, num_obs=BIG_WIDTH if nets not in NETS else 48, num_critic_obs=64)
    perm = torch.randperm(n * T, generator=torch.Generator().manual_seed(7))[:count].contiguous()
    assert len(perm) == count and int(perm.max()) < n * T and int(perm.min()) >= 0
    return ac, st, perm


@pytest.fixture(scope="module")
def grads_reference():
    """Per net: the float64 and float32 gradients and terms of every row count and loss type, computed once and left unchanged."""
    cache = {}

    def get(nets, row_cases=tuple(ROWS)):
        if (nets, row_cases) not in cache:
            cases = {}
            for rows in row_cases:
                ac, st, perm = _fixture(nets, rows)
                for lt in LOSS_TYPES:
                    cases[(rows, lt)] = (ref.grads_of(ac, lt, st, perm, torch.float64), ref.grads_of(ac, lt, st, perm, torch.float32))
            cache[(nets, row_cases)] = cases
        return cache[(nets, row_cases)]
    return get


def _to_device(ac, st):
    dev = ref.clone(ac, torch.float32).to(DEV)
    out = D.DistillStorage(st.n, st.T, DEV, ac.num_obs)
    for f in ("observations", "actions", "mu", "sigma", "teacher_actions", "dones"):
        getattr(out, f).copy_(getattr(st, f))
    return dev, out


def _device_grads(alg, dst, perm, loss_type):
    """One mpc_ppo_update_grads_distill on alg's handle: (the actor's gradients, the two terms) on the host."""
    alg._device_state(len(perm))
    alg._bind_storage(dst)
    idx = perm.to(DEV)
    terms = torch.zeros(2, device=DEV)
    P.check(P.update_lib().mpc_ppo_update_grads_distill(alg._handle, len(perm), idx.data_ptr(), D.LOSS_TYPES[loss_type], terms.data_ptr(), None), "grads_distill")
    return [p.grad.cpu().clone() for p in alg.actor_params()], terms.cpu().clone()


def _check_grads(cases, nets, rows, loss_type):
    gap = max(ref.rel_l2(g32, g64) for (g64s, _, _), (g32s, _, _) in cases.values() for g32, g64 in zip(g32s, g64s))
    rel = lambda x, r: abs(x - r) / abs(r)
    term_gap = max(rel(b[1][q], a[1][q]) for a, b in cases.values() for q in range(2))
    ac, st, perm = _fixture(nets, rows)
    (g64s, t64, share), _ = cases[(rows, loss_type)]
    if len(perm) > 1:
        assert 0.05 < share < 0.95, share                                         # both branches of huber's gradient are taken
    dev, dst = _to_device(ac, st)
    alg = D.Distillation(dev, D.DistillConfig(loss_type=loss_type), backend="hip")
    rest = [p for p in dev.bind_order()[len(alg.actor_params()):]]
    got, terms = _device_grads(alg, dst, perm, loss_type)
    what = f"{nets} {rows} {loss_type}"
    for q, name in enumerate(("behaviour loss", "mean |d|")):
        err = rel(float(terms[q]), t64[q])
        print(f"{what}: {name} {float(terms[q]):.9g} float64 {t64[q]:.9g}: off by {err:.3e} (bound {4 * term_gap:.3e}, ratio {err / term_gap:.3f})")
        assert term_gap > 0 and err <= 4 * term_gap, (name, err, term_gap)
    names = ref.actor_names(ac)
    ref.pooled([(names[k], ref.rel_l2(got[k], g64s[k]), gap) for k in range(len(names))], f"{what}: gradients")
    assert all(p.grad is None for p in rest)                                     # nothing of the critic's or std's was even made
    return alg, dst, perm, got, terms


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
@pytest.mark.parametrize("rows", sorted(ROWS))
@pytest.mark.parametrize("nets", sorted(NETS))
def test_grads_match_float64_autograd(grads_reference, nets, rows, loss_type):
    _check_grads(grads_reference(nets), nets, rows, loss_type)


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_grads_on_the_wide_tile_match_float64_autograd(grads_reference, loss_type):
    """8192 rows on the reference student: the smallest count at which a single-slot forward GEMM plans the 128 x 128 tile (64 x 4 tiles); layer 1's
    weight gradient and the backward-data GEMM into layer 0 take it too (tests/test_distill.py).  A pool of its own, over both loss types."""
    alg, dst, perm, got, terms = _check_grads(grads_reference("reference", ("big",)), "reference", "big", loss_type)
    again, terms2 = _device_grads(alg, dst, perm, loss_type)                     # and a rerun on the same handle is bit-identical
    assert all(torch.equal(a, b) for a, b in zip(got, again)) and torch.equal(terms, terms2)


def test_the_update_entry_points_refuse_before_the_device_is_touched():
    student, _ = _pair(48, 64)
    student._ready("test", _rows(1, 48, 1))
    L, err = P.update_lib(), lambda: P.update_lib().mpc_ppo_last_error()
    h = C.c_void_p()
    P.check(L.mpc_ppo_update_create(C.byref(h), student._handle, 64), "create")
    try:
        idx, terms, lr = torch.zeros(64, dtype=torch.long, device=DEV), torch.zeros(2, device=DEV), torch.full((1,), 1e-3, dtype=torch.float64, device=DEV)
        grads = lambda rows=4, loss=0: L.mpc_ppo_update_grads_distill(h, rows, idx.data_ptr(), loss, terms.data_ptr(), None)
        apply = lambda: L.mpc_ppo_update_apply_actor(h, 1.0, 0.9, 0.999, 1e-8, 1, lr.data_ptr(), None)
        for rows in (0, -1, 65):
            assert grads(rows=rows) == -1 and b"rows must lie in 1 .. max_rows" in err()
        for loss in (-1, 2):
            assert grads(loss=loss) == -1 and b"loss_type is 0 (mse) or 1 (huber)" in err()
        assert grads() == -1 and b"no gradients bound" in err()
        assert apply() == -1 and b"no gradients and moments bound" in err()
        params = student.bind_order()
        g = [torch.zeros_like(p) for p in params]
        arr = _lib.ptr_array([t.data_ptr() for t in g])
        P.check(L.mpc_ppo_update_bind(h, arr, None, None), "bind")
        assert grads() == -1 and b"no storage set" in err()
        assert apply() == -1 and b"no gradients and moments bound" in err()     # gradients alone
        st = D.DistillStorage(8, 8, DEV, 48)
        flag = st.dones.data_ptr()
        P.check(L.mpc_ppo_update_set_storage(h, 64, st.observations.data_ptr(), st.actions.data_ptr(), flag, flag, flag, flag, st.mu.data_ptr(), st.sigma.data_ptr()), "storage")
        assert grads() == -1 and b"no targets set" in err()
        assert L.mpc_ppo_update_set_distill_targets(h, st.teacher_actions.data_ptr() + 4) == -1 and b"16-byte aligned" in err()
        P.check(L.mpc_ppo_update_set_distill_targets(h, st.teacher_actions.data_ptr()), "targets")
        P.check(L.mpc_ppo_update_set_distill_targets(h, None), "targets")        # cleared
        assert grads() == -1 and b"no targets set" in err()
        for a in (dict(max_norm=0.0), dict(beta1=1.0), dict(step=0)):
            v = {**dict(max_norm=1.0, beta1=0.9, step=1), **a}
            assert L.mpc_ppo_update_apply_actor(h, v["max_norm"], v["beta1"], 0.999, 1e-8, v["step"], lr.data_ptr(), None) == -1 and b"mpc_ppo_update_apply_actor" in err()
        torch.cuda.synchronize()
        assert all(float(t.abs().max()) == 0 for t in g) and float(terms.abs().max()) == 0          # nothing ran
    finally:
        L.mpc_ppo_update_destroy(h)


# ---- the clip and Adam over the actor alone
@pytest.mark.parametrize("max_norm", (0.01, 1e3))
def test_apply_actor_matches_clip_and_adam_and_leaves_the_rest(grads_reference, max_norm):
    """Three steps over the float32 gradients of three cases, on a handle bound as PPO binds it: every tensor of the mpc_ac with a gradient and both
    moments.  The critic's and std's are pre-filled with patterns and must come back bit for bit -- also from mpc_ppo_update_grads_distill, run in
    between on the same handle."""
    nets = "uneven"
    cases = grads_reference(nets)
    ac, st, perm = _fixture(nets, "ragged")
    grads = [[g.float() for g in cases[(rows, "mse")][0][0]] for rows in ("ragged", "two heads", "chunked")]
    norms = [float(torch.cat([g.flatten() for g in gs]).norm()) for gs in grads]
    assert all(0.01 < x < 1e3 for x in norms), norms                               # 0.01 always clips, 1e3 never
    runs = {(m, dt): ref.apply_steps(ac, grads, m, 1e-3, dt) for m in (0.01, 1e3) for dt in (torch.float32, torch.float64)}
    names, n_actor = ref.actor_names(ac), len(ref.actor_params(ac))
    p0 = [p.detach().double() for p in ref.actor_params(ac)]
    gaps = {}
    for m in (0.01, 1e3):
        for s in range(3):
            for kind in range(3):
                for k in range(n_actor):
                    off = p0[k] if kind == 0 else 0.0
                    gaps[kind] = max(gaps.get(kind, 0.0), ref.rel_l2(runs[(m, torch.float32)][s][kind][k].double() - off, runs[(m, torch.float64)][s][kind][k] - off))
    dev, dst = _to_device(ac, st)
    alg = P.PPO(dev, P.PPOConfig(actor_hidden_dims=NETS[nets][0], critic_hidden_dims=NETS[nets][1]), backend="hip")
    alg._device_state(len(perm))
    params = dev.bind_order()
    rest = params[n_actor:]
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in rest:                                                           # a student that carries PPO's gradients and moments
            p.grad.copy_(torch.randn(p.shape, generator=g))
            alg.optimizer.state[p]["exp_avg"].copy_(torch.randn(p.shape, generator=g) * 0.1)
            alg.optimizer.state[p]["exp_avg_sq"].copy_(torch.rand(p.shape, generator=g) * 0.1 + 0.01)
    snapshot = lambda: [t.detach().clone() for p in rest for t in (p, p.grad, alg.optimizer.state[p]["exp_avg"], alg.optimizer.state[p]["exp_avg_sq"])]
    before = snapshot()
    assert all(float(t.abs().min()) > 0 for t in before)
    L = P.update_lib()
    flag = dst.dones.data_ptr()
    P.check(L.mpc_ppo_update_set_storage(alg._handle, dst.n * dst.T, dst.observations.data_ptr(), dst.actions.data_ptr(), flag, flag, flag, flag,
                                         dst.mu.data_ptr(), dst.sigma.data_ptr()), "storage")
    P.check(L.mpc_ppo_update_set_distill_targets(alg._handle, dst.teacher_actions.data_ptr()), "targets")
    idx, terms = perm.to(DEV), torch.zeros(2, device=DEV)
    alg.lr_device.fill_(1e-3)
    for s in range(3):
        P.check(L.mpc_ppo_update_grads_distill(alg._handle, len(perm), idx.data_ptr(), 0, terms.data_ptr(), None), "grads_distill")
        assert all(float(p.grad.abs().max()) > 0 for p in params[:n_actor])
        for p, x in zip(params[:n_actor], grads[s]):
            p.grad.copy_(x)
        P.check(L.mpc_ppo_update_apply_actor(alg._handle, max_norm, 0.9, 0.999, 1e-8, s + 1, alg.lr_device.data_ptr(), None), "apply_actor")
        want = runs[(max_norm, torch.float64)][s]
        state = [params[:n_actor], [alg.optimizer.state[p]["exp_avg"] for p in params[:n_actor]], [alg.optimizer.state[p]["exp_avg_sq"] for p in params[:n_actor]]]
        for kind, what in enumerate(("parameter change", "exp_avg", "exp_avg_sq")):
            errs = []
            for k in range(n_actor):
                off = p0[k] if kind == 0 else 0.0
                errs.append((names[k], ref.rel_l2(state[kind][k].detach().cpu().double() - off, want[kind][k] - off), gaps[kind]))
            ref.pooled(errs, f"max_norm {max_norm} step {s + 1}: {what}")
    assert all(torch.equal(a, b) for a, b in zip(before, snapshot()))           # the critic, std, their gradients and moments: untouched


# ---- the whole update
def _hip_update(ac, st, perm, loss_type, backend="hip"):
    dev, dst = _to_device(ac, st)
    alg = D.Distillation(dev, D.DistillConfig(num_learning_epochs=2, num_mini_batches=4, loss_type=loss_type, actor_hidden_dims=NETS["uneven"][0],
                                              critic_hidden_dims=NETS["uneven"][1]), backend=backend)
    out = alg.update(dst, indices=perm.to(DEV))
    return dev, alg, out


@pytest.fixture(scope="module")
def chained_reference():
    ac, st = ref.fixture(NETS["uneven"], 65, 6)
    perm = torch.randperm(390, generator=torch.Generator().manual_seed(7))[:4 * 97].contiguous()
    runs = {}
    for lt in LOSS_TYPES:
        cfg = D.DistillConfig(num_learning_epochs=1, num_mini_batches=4, loss_type=lt)
        runs[lt] = (ref.update(ac, cfg, st, perm, torch.float64), ref.update(ac, cfg, st, perm, torch.float32))
    return ac, st, perm, runs


def test_rerun_is_bit_identical(chained_reference):
    ac, st, perm, _ = chained_reference
    a, b = _hip_update(ac, st, perm, "huber"), _hip_update(ac, st, perm, "huber")
    for x, y in zip(a[0].bind_order(), b[0].bind_order()):
        assert torch.equal(x, y)
    for x, y in zip(a[1].actor_params(), b[1].actor_params()):
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a[1].optimizer.state[x][key], b[1].optimizer.state[y][key])
        assert int(a[1].optimizer.state[x]["step"]) == 8 and not a[1].optimizer.state[x]["step"].is_cuda
    assert torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1]) and all(torch.equal(x, y) for x, y in zip(a[1].last_terms, b[1].last_terms))
    assert not torch.equal(a[0].actor[0].weight.cpu(), ac.actor[0].weight) and torch.equal(a[0].critic[0].weight.cpu(), ac.critic[0].weight)
    assert torch.equal(a[0].std.cpu(), ac.std.detach())


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_the_backends_first_updates_agree(chained_reference, loss_type):
    """One epoch of four mini-batches from one state on one storage with one permutation: either backend's actor is within the rule of the float64
    restatement (the gaps pooled over the tensors and both loss types), so the two agree within twice the bound; and neither moved the rest."""
    ac, st, perm, runs = chained_reference
    n_actor, names = len(ref.actor_params(ac)), ref.actor_names(ac)
    p0 = [p.detach().double() for p in ac.bind_order()]
    gaps = {}
    for r64, r32 in runs.values():
        for kind, (a64, a32) in enumerate(((r64[0][:n_actor], r32[0][:n_actor]), (r64[2], r32[2]), (r64[3], r32[3]))):
            for k in range(n_actor):
                off = p0[k] if kind == 0 else 0.0
                gaps[kind] = max(gaps.get(kind, 0.0), ref.rel_l2(a32[k].double() - off, a64[k] - off))
    r64 = runs[loss_type][0]
    means = lambda run: [np.mean([t[q] for t in run[1]]) for q in range(2)]
    pool = max(abs(a - b) / abs(b) for x64, x32 in runs.values() for a, b in zip(means(x32), means(x64)))
    for backend in D.BACKENDS:
        dev, dst = _to_device(ac, st)
        alg = D.Distillation(dev, D.DistillConfig(num_learning_epochs=1, num_mini_batches=4, loss_type=loss_type), backend=backend)
        loss, gap = alg.update(dst, indices=perm.to(DEV))
        params = dev.bind_order()
        state = [params[:n_actor], [alg.optimizer.state[p]["exp_avg"] for p in params[:n_actor]], [alg.optimizer.state[p]["exp_avg_sq"] for p in params[:n_actor]]]
        for kind, what in enumerate(("parameter change", "exp_avg", "exp_avg_sq")):
            want = (r64[0][:n_actor], r64[2], r64[3])[kind]
            errs = []
            for k in range(n_actor):
                off = p0[k] if kind == 0 else 0.0
                errs.append((names[k], ref.rel_l2(state[kind][k].detach().cpu().double() - off, want[k] - off), gaps[kind]))
            ref.pooled(errs, f"{backend} {loss_type}: {what}")
        for name, got, want in zip(("behaviour loss", "action gap"), (float(loss), float(gap)), means(r64)):
            print(f"{backend} {loss_type}: returned mean {name} {got:.9g} float64 {want:.9g} (bound {4 * pool:.3e})")
            assert pool > 0 and abs(got - want) <= 4 * pool * abs(want)
        assert all(torch.equal(p.detach().cpu(), q.detach()) for p, q in zip(params[n_actor:], ac.bind_order()[n_actor:]))
        assert set(alg.optimizer.state_dict()["state"]) == set(range(n_actor))      # the checkpoint: the actor's tensors, whichever backend wrote it


def test_update_never_waits(chained_reference):
    ac, st, perm, _ = chained_reference
    dev, dst = _to_device(ac, st)
    alg = D.Distillation(dev, D.DistillConfig(num_learning_epochs=2, num_mini_batches=4), backend="hip")
    idx = perm.to(DEV)
    alg.update(dst, indices=idx)                                                 # (the first update creates the handle and the optimiser state)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")        # a torch call that waits for the device or copies to the host raises from here on
    try:
        alg.update(dst, indices=idx)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    alg.update(dst)                                                              # and with its own randperm
    assert all(int(alg.optimizer.state[p]["step"]) == 24 for p in alg.actor_params())


# ---- end to end: teacher, distillation, fine-tuning, deployment
def test_teacher_distillation_and_fine_tuning_end_to_end(tmp_path):
    from tests.test_ppo_asymmetric_gpu import N_ENVS, _finite, _task
    T, hidden = 8, dict(actor_hidden_dims=(64, 32), critic_hidden_dims=(32,))
    task = _task()
    wp = task.num_privileged_obs
    assert N_ENVS == 64 and wp == 240
    # 1. a teacher whose actor reads the privileged rows, trained by the unchanged trainer
    teacher = P.PPOTrainer(D.TeacherEnv(task), P.PPOConfig(num_steps_per_env=T, num_learning_epochs=1, num_mini_batches=2, init_noise_std=0.5, **hidden), seed=3)
    assert teacher.actor_critic.actor[0].weight.shape == (64, wp) and teacher.actor_critic.num_critic_obs == wp
    assert _finite(teacher.learn(1))
    assert torch.equal(teacher.storage.observations, teacher.storage.privileged_observations)      # the actor read the critic's rows
    teacher_path, student_path = str(tmp_path / "teacher.pt"), str(tmp_path / "student.pt")
    teacher.save(teacher_path)
    # 2. the student: labelled rollouts, the device update
    cfg = D.DistillConfig(num_steps_per_env=T, num_learning_epochs=2, num_mini_batches=2, **hidden)
    d = D.Distiller(task, teacher_path, cfg, seed=5, update="hip")
    ac = d.actor_critic
    assert ac.num_obs == task.num_obs and ac.num_critic_obs == wp and float(ac.std.detach().min()) == float(ac.std.detach().max()) == np.float32(0.1)
    assert all(torch.equal(a, b.to(DEV)) for a, b in zip(d.teacher.state_dict().values(), torch.load(teacher_path)["model_state_dict"].values()))
    critic0, std0 = [p.detach().clone() for p in ac.critic.parameters()], ac.std.detach().clone()
    infos = d.learn(3)
    assert [i["iter"] for i in infos] == [1, 2, 3] and _finite(infos)
    assert all(i["behavior_loss"] > 0 and i["action_gap"] > 0 and "mean_reward" in i and "mean_episode_return" in i and "episodes_finished" in i for i in infos)
    st = d.storage
    assert float(st.teacher_actions.abs().max()) > 0 and float(st.dones.max()) == 1.0 and bool(((st.dones == 0) | (st.dones == 1)).all())
    assert all(torch.equal(a, b) for a, b in zip(critic0, ac.critic.parameters())) and torch.equal(std0, ac.std)
    assert all(torch.equal(a, b.to(DEV)) for a, b in zip(d.teacher.state_dict().values(), torch.load(teacher_path)["model_state_dict"].values()))      # never written
    # on a storage held fixed, ten updates bring the loss below its first value
    first = float(d.alg.update(st)[0])
    for _ in range(9):
        last = float(d.alg.update(st)[0])
    print(f"behaviour loss on the held storage: {first:.6g} -> {last:.6g}; records {[round(i['behavior_loss'], 6) for i in infos]}")
    assert last < first
    d.save(student_path)
    # 3. the checkpoint: fine-tuning by the unchanged trainer, and deployment
    obs = st.observations[0].contiguous()
    want = ac.act_inference(obs)
    tuned = P.PPOTrainer(task, P.PPOConfig(num_steps_per_env=T, num_learning_epochs=1, num_mini_batches=2, **hidden), seed=7, update="hip")
    tuned.load(student_path, load_optimizer=False)
    assert torch.equal(tuned.actor_critic.act_inference(obs), want) and tuned.iteration == 3
    raw = WeightPolicy.from_state_dict(torch.load(student_path)["model_state_dict"], device=DEV).step(obs, return_actions=True)[1]
    assert torch.equal(raw, want)
    assert _finite(tuned.learn(1)) and not torch.equal(tuned.actor_critic.act_inference(obs), want)
    # a distiller resumes from its own checkpoint, optimiser included, on either backend
    other = D.Distiller(task, d.teacher, cfg, seed=6, update="torch")
    other.load(student_path)
    assert torch.equal(other.get_inference_policy()(obs), want) and other.iteration == 3
    sa, sb = d.alg.optimizer.state_dict()["state"], other.alg.optimizer.state_dict()["state"]
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k][m], sb[k][m]) for k in sa for m in ("exp_avg", "exp_avg_sq"))
    assert _finite(other.learn(1)) and other.iteration == 4
