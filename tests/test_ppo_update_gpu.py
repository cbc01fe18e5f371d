"""The device PPO update on the MI355X (include/mpc_ppo_update.h, rl_mpc_locomotion_amd.ppo.PPO(backend="hip")) against torch autograd +
torch.optim.Adam in float64 on the CPU (tests/ppo_update_ref.py), on the same storage, indices and hyper-parameters.

The tolerance is the project's rule: at most 4 x the distance of torch's own float32 run from the float64 run, which this module computes.  The
distance is pooled, because a single tensor's is one draw of a rounding error: gradients, parameter changes and moments are compared tensor by
tensor in relative L2, each held to 4 x the largest per-tensor gap over all row-count cases (and mini-batches, steps) of the same net pair; the
scalar terms as tests/test_ppo_update.py pools them, over the same cases.  Largest measured ratios error / gap: DESIGN.md section 8.3.

Those row counts all plan the 128 x 64 tile and 256-row weight-gradient chunks (csrc/ppo_gemm_plan.h).  BIG_ROWS x BIG_NETS are the cases that reach what
the training workload runs -- the 128 x 128 tile in all three kinds and chunks of 1024 and 512 rows -- with a pool of their own, so the cases above keep
their gaps; tests/test_ppo_gemm_plan.py pins which kernel each of this module's shapes reaches."""
import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import ppo as P
from tests import ppo_update_ref as ref
from tests.test_policy import ACT_ATOL, ACT_RTOL
from tests.test_ppo import _filled_storage
from tests.test_ppo_gpu import _Standin, _obs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NETS = {"reference": ((512, 256, 128), (512, 256, 128)), "uneven": ((32, 16), (64,)), "odd": ((80, 48), (144,))}
ROWS = {"single": (1, 1, 1), "ragged": (65, 6, 4), "chunked": (65, 16, 1)}        # n, T, mini-batches: 1 row; 4 x 97 rows, 2 left out; 1040 rows
BIG_NETS = {"reference": NETS["reference"], "square": ((256, 256), (256, 256))}
BIG_ROWS = {"production": (3277, 5, 1)}                                           # 16 385 rows in one mini-batch: 17 chunks of 1024, 33 of 512, the last of 1 row
ALL_NETS, ALL_ROWS = {**NETS, **BIG_NETS}, {**ROWS, **BIG_ROWS}
DESIRED_KL = (0.01, 0.06, 1.0)                                                    # first-step kl 0.048 .. 0.076: down, unchanged, up


def _cfg(nets, mini_batches=1, **kw):
    return P.PPOConfig(actor_hidden_dims=ALL_NETS[nets][0], critic_hidden_dims=ALL_NETS[nets][1], init_noise_std=0.7, num_mini_batches=mini_batches, **kw)


def _fixture(nets, rows):
    """(CPU actor-critic, CPU storage, injected permutation) as tests/test_ppo.py builds them."""
    n, T, mb = ALL_ROWS[rows]
    torch.manual_seed(5)
    ac = P.ActorCritic(48, 12, *ALL_NETS[nets], init_noise_std=0.7)
    st = _filled_storage(ac, n=n, T=T, seed=6)
    size = n * T // mb
    perm = torch.randperm(n * T, generator=torch.Generator().manual_seed(7))[:mb * size].contiguous()
    return ac, st, perm


def _to_device(ac, st):
    dev = ref.clone(ac, torch.float32).to(DEV)
    out = P.RolloutStorage(st.n, st.T, DEV)
    for f in ref.FIELDS:
        getattr(out, f).copy_(getattr(st, f))
    out.step = out.T
    return dev, out


def _pooled(errs_and_gaps, what):
    """errs_and_gaps: (name, error, gap) per tensor.  Every error within 4 x the largest gap; returns the largest ratio."""
    gap = max(g for _, _, g in errs_and_gaps)
    worst = max(errs_and_gaps, key=lambda x: x[1])
    print(f"{what}: largest error {worst[1]:.3e} ({worst[0]}), largest gap {gap:.3e}, ratio {worst[1] / gap:.3f}")
    assert gap > 0
    for name, err, _ in errs_and_gaps:
        assert err <= 4 * gap, f"{what}: {name} off by {err:.3e} > 4 x {gap:.3e}"
    return worst[1] / gap


@pytest.fixture(scope="module")
def grads_reference():
    """Per net pair: float64 and float32 gradients and terms of every mini-batch of every row-count case, computed once."""
    cache = {}

    def get(nets):
        if nets not in cache:
            cases = {}
            for rows in ROWS:
                ac, st, perm = _fixture(nets, rows)
                mb = ROWS[rows][2]
                size = len(perm) // mb
                cfg = _cfg(nets, mb)
                cases[rows] = [(ref.grads_of(ac, cfg, st, perm[i * size:(i + 1) * size], torch.float64),
                                ref.grads_of(ac, cfg, st, perm[i * size:(i + 1) * size], torch.float32)) for i in range(mb)]
            cache[nets] = cases
        return cache[nets]
    return get


def _names(ac):
    la, lc = len(ac._linears(ac.actor)), len(ac._linears(ac.critic))
    return [f"actor W{l}" for l in range(la)] + [f"actor b{l}" for l in range(la)] + [f"critic W{l}" for l in range(lc)] + [f"critic b{l}" for l in range(lc)] + ["std"]


@pytest.mark.parametrize("rows", sorted(ROWS))
@pytest.mark.parametrize("nets", sorted(NETS))
def test_grads_match_float64_autograd(grads_reference, nets, rows):
    cases = grads_reference(nets)
    gap = max(ref.rel_l2(g32, g64) for case in cases.values() for (g64s, _, _), (g32s, _, _) in case for g32, g64 in zip(g32s, g64s))
    ac, st, perm = _fixture(nets, rows)
    mb = ROWS[rows][2]
    size = len(perm) // mb
    dev, dst = _to_device(ac, st)
    names = _names(ac)
    for kl_i, desired in enumerate(DESIRED_KL):
        alg = P.PPO(dev, _cfg(nets, mb, desired_kl=desired), backend="hip")
        alg._device_state(size)
        L = P.update_lib()
        flat = [getattr(dst, f) for f in ref.FIELDS]
        P.check(L.mpc_ppo_update_set_storage(alg._handle, dst.n * dst.T, *[t.data_ptr() for t in flat]), "set_storage")
        idx = perm.to(DEV)
        terms = torch.zeros(4, device=DEV)
        for i in range(mb if kl_i == 0 else 1):
            (g64s, t64, frac), (g32s, t32, _) = cases[rows][i]
            if rows != "single":
                assert 0.05 < frac[0] < 0.95 and 0.05 < frac[1] < 0.95, frac
            else:
                assert frac == (1.0, 1.0)
            alg.lr_device.fill_(1e-3)
            c = alg.cfg
            P.check(L.mpc_ppo_update_grads(alg._handle, size, idx.data_ptr() + 8 * i * size, c.clip_param, c.value_loss_coef, c.entropy_coef, 1, 1, desired,
                                           alg.lr_device.data_ptr(), terms.data_ptr(), None), "grads")
            got = [p.grad.cpu() for p in dev.bind_order()]
            assert float(alg.lr_device) == ref.adapt(1e-3, t64[3], c), (desired, t64[3])
            if kl_i:
                continue
            # the terms: pooled over this net pair's cases as test_ppo_update.check_terms pools them
            rel = lambda x, r: abs(x - r) / abs(r)
            pool3 = max(rel(b[1][q], a[1][q]) for case in cases.values() for a, b in case for q in range(3))
            pool_kl = max(rel(b[1][3], a[1][3]) for case in cases.values() for a, b in case)
            for q, name in enumerate(("surrogate", "value loss", "entropy", "kl")):
                g = pool_kl if q == 3 else pool3
                err = rel(float(terms[q]), t64[q])
                print(f"{nets} {rows} mini-batch {i}: {name} off by {err:.3e} (bound {4 * g:.3e}, ratio {err / g:.3f})")
                assert g > 0 and err <= 4 * g, (name, err, g)
            errs = [(names[k], ref.rel_l2(got[k], g64s[k]), gap) for k in range(len(names))]
            _pooled(errs, f"{nets} {rows} mini-batch {i}: gradients")
    # the schedule is skipped for a fixed one
    alg.lr_device.fill_(1e-3)
    P.check(L.mpc_ppo_update_grads(alg._handle, size, idx.data_ptr(), 0.2, 1.0, 0.01, 1, 0, 0.0, None, terms.data_ptr(), None), "grads")
    assert float(alg.lr_device) == 1e-3


@pytest.fixture(scope="module")
def big_reference():
    """Per net pair and BIG_ROWS case: the fixture and the float64 and float32 gradients and terms of its one mini-batch, computed once."""
    cache = {}

    def get(nets):
        if nets not in cache:
            cases = {}
            for rows in BIG_ROWS:
                assert BIG_ROWS[rows][2] == 1
                ac, st, perm = _fixture(nets, rows)
                cfg = _cfg(nets, 1, desired_kl=0.06)
                cases[rows] = (ac, st, perm, ref.grads_of(ac, cfg, st, perm, torch.float64), ref.grads_of(ac, cfg, st, perm, torch.float32))
            cache[nets] = cases
        return cache[nets]
    return get


def _device_grads(alg, dst, perm, size):
    """One mpc_ppo_update_grads over the first `size` rows of perm on alg's handle: (gradients, terms, learning rate) on the host."""
    L = P.update_lib()
    P.check(L.mpc_ppo_update_set_storage(alg._handle, dst.n * dst.T, *[getattr(dst, f).data_ptr() for f in ref.FIELDS]), "set_storage")
    idx = perm.to(DEV)
    terms = torch.zeros(4, device=DEV)
    alg.lr_device.fill_(1e-3)
    c = alg.cfg
    P.check(L.mpc_ppo_update_grads(alg._handle, size, idx.data_ptr(), c.clip_param, c.value_loss_coef, c.entropy_coef, 1, 1, c.desired_kl,
                                   alg.lr_device.data_ptr(), terms.data_ptr(), None), "grads")
    return [p.grad.cpu().clone() for p in alg.actor_critic.bind_order()], terms.cpu().clone(), float(alg.lr_device)


@pytest.mark.parametrize("rows", sorted(BIG_ROWS))
@pytest.mark.parametrize("nets", sorted(BIG_NETS))
def test_grads_on_the_production_plan_match_float64_autograd(big_reference, nets, rows):
    """test_grads_match_float64_autograd's rule (desired_kl = 0.06) at a row count that plans the wide tile and the long chunks; the float32 gap is
    pooled over the BIG_ROWS cases of this net pair only."""
    cases = big_reference(nets)
    gap = max(ref.rel_l2(g32, g64) for _, _, _, (g64s, _, _), (g32s, _, _) in cases.values() for g32, g64 in zip(g32s, g64s))
    rel = lambda x, r: abs(x - r) / abs(r)
    pool3 = max(rel(b[1][q], a[1][q]) for _, _, _, a, b in cases.values() for q in range(3))
    pool_kl = max(rel(b[1][3], a[1][3]) for _, _, _, a, b in cases.values())
    ac, st, perm, (g64s, t64, frac), _ = cases[rows]
    assert 0.05 < frac[0] < 0.95 and 0.05 < frac[1] < 0.95, frac
    dev, dst = _to_device(ac, st)
    alg = P.PPO(dev, _cfg(nets, 1, desired_kl=0.06), backend="hip")
    alg._device_state(len(perm))
    got, terms, lr = _device_grads(alg, dst, perm, len(perm))
    assert lr == ref.adapt(1e-3, t64[3], alg.cfg), t64[3]
    for q, name in enumerate(("surrogate", "value loss", "entropy", "kl")):
        g = pool_kl if q == 3 else pool3
        err = rel(float(terms[q]), t64[q])
        print(f"{nets} {rows}: {name} off by {err:.3e} (bound {4 * g:.3e}, ratio {err / g:.3f})")
        assert g > 0 and err <= 4 * g, (name, err, g)
    names = _names(ac)
    for k in range(len(names)):
        print(f"{nets} {rows}: {names[k]} off by {ref.rel_l2(got[k], g64s[k]):.3e}, its own float32 gap {ref.rel_l2(cases[rows][4][0][k], g64s[k]):.3e}")
    _pooled([(names[k], ref.rel_l2(got[k], g64s[k]), gap) for k in range(len(names))], f"{nets} {rows}: gradients")


@pytest.mark.parametrize("nets", sorted(BIG_NETS))
def test_a_smaller_batch_on_a_used_handle_reads_no_stale_workspace(big_reference, nets):
    """The 1040-row case on a handle that has just run 16 385 rows (rows < max_rows: the workspace still holds that run's longer activations and
    more chunk partials) is bit-identical to the same call on a fresh handle made for 1040 rows."""
    ac, st, perm, _, _ = big_reference(nets)["production"]
    small_ac, small_st, small_perm = _fixture(nets, "chunked")
    assert all(torch.equal(a, b) for a, b in zip(ac.bind_order(), small_ac.bind_order()))         # the same nets with the same weights
    rows = len(small_perm)
    assert rows == 1040 < len(perm)
    dev, dst = _to_device(ac, st)
    _, small_dst = _to_device(small_ac, small_st)
    used = P.PPO(dev, _cfg(nets, 1, desired_kl=0.06), backend="hip")
    used._device_state(len(perm))
    handle = used._handle.value
    _device_grads(used, dst, perm, len(perm))
    used._device_state(rows)
    assert used._handle.value == handle and used._max_rows == len(perm)                         # the handle of the large run, not a new one
    a = _device_grads(used, small_dst, small_perm, rows)
    fresh_dev, _ = _to_device(small_ac, small_st)
    fresh = P.PPO(fresh_dev, _cfg(nets, 1, desired_kl=0.06), backend="hip")
    fresh._device_state(rows)
    assert fresh._max_rows == rows
    b = _device_grads(fresh, small_dst, small_perm, rows)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert all(float(g.abs().max()) > 0 for g in a[0])


@pytest.fixture(scope="module")
def apply_reference(grads_reference):
    cache = {}

    def get(nets):
        if nets not in cache:
            ac, _, _ = _fixture(nets, "ragged")
            grads = [[g.float() for g in case[0][0]] for case in grads_reference(nets)["ragged"][:3]]       # float32 gradients of mini-batches 0 .. 2
            norms = [float(torch.cat([g.flatten() for g in gs]).norm()) for gs in grads]
            cache[nets] = (ac, grads, norms, {(m, dt): ref.apply_steps(ac, grads, m, 1e-3 / 1.5, dt) for m in (0.25, 1e3) for dt in (torch.float32, torch.float64)})
        return cache[nets]
    return get


@pytest.mark.parametrize("max_norm", (0.25, 1e3))
@pytest.mark.parametrize("nets", sorted(NETS))
def test_apply_matches_clip_and_adam(apply_reference, nets, max_norm):
    ac, grads, norms, runs = apply_reference(nets)
    assert all(0.25 < x < 1e3 for x in norms), norms                               # 0.25 always clips, 1e3 never
    p0 = [p.detach().clone() for p in ac.bind_order()]
    names = _names(ac)
    gaps = {}
    for (m, dt), run in runs.items():
        if dt == torch.float64:
            continue
        for s in range(3):
            for kind in range(3):
                for k in range(len(names)):
                    a, b = run[s][kind][k].double(), runs[(m, torch.float64)][s][kind][k]
                    if kind == 0:
                        a, b = a - p0[k].double(), b - p0[k].double()
                    gaps[kind] = max(gaps.get(kind, 0.0), ref.rel_l2(a, b))
    dev = ref.clone(ac, torch.float32).to(DEV)
    alg = P.PPO(dev, _cfg(nets, max_grad_norm=max_norm), backend="hip")
    alg.set_learning_rate(1e-3 / 1.5)
    alg._device_state(8)
    L = P.update_lib()
    params = dev.bind_order()
    for s in range(3):
        for p, g in zip(params, grads[s]):
            p.grad.copy_(g)
        P.check(L.mpc_ppo_update_apply(alg._handle, max_norm, 0.9, 0.999, 1e-8, s + 1, alg.lr_device.data_ptr(), None), "apply")
        want = runs[(max_norm, torch.float64)][s]
        state = [params, [alg.optimizer.state[p]["exp_avg"] for p in params], [alg.optimizer.state[p]["exp_avg_sq"] for p in params]]
        for kind, what in enumerate(("parameter change", "exp_avg", "exp_avg_sq")):
            errs = []
            for k in range(len(names)):
                a, b = state[kind][k].detach().cpu().double(), want[kind][k]
                if kind == 0:
                    a, b = a - p0[k].double(), b - p0[k].double()
                errs.append((names[k], ref.rel_l2(a, b), gaps[kind]))
            _pooled(errs, f"{nets} max_norm {max_norm} step {s + 1}: {what}")


@pytest.fixture(scope="module")
def chained_reference():
    ac, st, perm = _fixture("uneven", "ragged")
    runs = {}
    for desired in DESIRED_KL:
        cfg = _cfg("uneven", 4, desired_kl=desired, num_learning_epochs=2)
        runs[desired] = (ref.update(ac, cfg, st, perm, torch.float64), ref.update(ac, cfg, st, perm, torch.float32))
    return ac, st, perm, runs


def _hip_update(ac, st, perm, desired):
    dev, dst = _to_device(ac, st)
    alg = P.PPO(dev, _cfg("uneven", 4, desired_kl=desired, num_learning_epochs=2), backend="hip")
    alg.record_lr = True
    out = alg.update(dst, indices=perm.to(DEV))
    return dev, dst, alg, out


@pytest.mark.parametrize("desired", DESIRED_KL)
def test_chained_update_follows_the_float64_schedule(chained_reference, desired):
    ac, st, perm, runs = chained_reference
    (p64, lrs64, terms64, m64, v64), (p32, lrs32, _, m32, v32) = runs[desired]
    assert lrs32 == lrs64 and len(lrs64) == 8                                      # torch's own two runs decide alike: the sequence is comparable
    dev, dst, alg, (mean_value, mean_surrogate) = _hip_update(ac, st, perm, desired)
    assert alg.lr_trace.tolist() == lrs64, (alg.lr_trace.tolist(), lrs64)
    assert float(alg.lr_device) == lrs64[-1] and dst.step == 0
    if desired == 0.01:
        assert lrs64[0] < 1e-3
    elif desired == 1.0:
        assert lrs64[0] > 1e-3
    else:
        assert lrs64[0] == 1e-3
    p0 = [p.detach().double() for p in ac.bind_order()]
    names = _names(ac)
    params = dev.bind_order()
    state = [params, [alg.optimizer.state[p]["exp_avg"] for p in params], [alg.optimizer.state[p]["exp_avg_sq"] for p in params]]
    for kind, what in enumerate(("parameter change", "exp_avg", "exp_avg_sq")):
        gap = 0.0
        for d in DESIRED_KL:                                                       # pooled over the three schedules of this net pair
            r64, r32 = runs[d]
            a64, a32 = (r64[0], r64[3], r64[4])[kind], (r32[0], r32[3], r32[4])[kind]
            for k in range(len(names)):
                off = p0[k] if kind == 0 else 0.0
                gap = max(gap, ref.rel_l2(a32[k].double() - off, a64[k] - off))
        want = (p64, m64, v64)[kind]
        errs = []
        for k in range(len(names)):
            off = p0[k] if kind == 0 else 0.0
            errs.append((names[k], ref.rel_l2(state[kind][k].detach().cpu().double() - off, want[k] - off), gap))
        _pooled(errs, f"chained, desired_kl {desired}: {what}")
    # the returned means (value loss, surrogate) over the eight mini-batches: the two scalars pooled over the three schedules
    means = lambda run: (np.mean([t[1] for t in run[2]]), np.mean([t[0] for t in run[2]]))
    gap = max(abs(a - b) / abs(b) for d in DESIRED_KL for a, b in zip(means(runs[d][1]), means(runs[d][0])))
    for got, want in zip((float(mean_value), float(mean_surrogate)), means(runs[desired][0])):
        print(f"chained, desired_kl {desired}: returned mean {got:.9g} float64 {want:.9g} (bound {4 * gap:.3e})")
        assert gap > 0 and abs(got - want) <= 4 * gap * abs(want)
    assert all(int(alg.optimizer.state[p]["step"]) == 8 and not alg.optimizer.state[p]["step"].is_cuda for p in params)


def test_rerun_is_bit_identical(chained_reference):
    ac, st, perm, _ = chained_reference
    a, b = _hip_update(ac, st, perm, 0.01), _hip_update(ac, st, perm, 0.01)
    for x, y in zip(a[0].bind_order(), b[0].bind_order()):
        assert torch.equal(x, y)
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a[2].optimizer.state[x][key], b[2].optimizer.state[y][key])
    assert all(torch.equal(x, y) for x, y in zip(a[2].last_terms, b[2].last_terms)) and torch.equal(a[2].lr_trace, b[2].lr_trace)
    assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1])


def test_update_never_waits_and_act_sees_the_new_weights(chained_reference):
    ac, st, perm, _ = chained_reference
    dev, dst = _to_device(ac, st)
    alg = P.PPO(dev, _cfg("uneven", 4, num_learning_epochs=2), backend="hip")
    obs = _obs(33, seed=4)
    before = dev.act(obs, seed=1, step=0)
    ptrs = dev._bound_ptrs
    idx = perm.to(DEV)
    alg.update(dst, indices=idx)                                                 # (the first update creates the handle and the optimiser state)
    dst.step = dst.T
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")        # a torch call that waits for the device or copies to the host raises from here on
    try:
        alg.update(dst, indices=idx)
        after = dev.act(obs, seed=1, step=0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    dst.step = dst.T
    alg.update(dst)                                                              # and with its own randperm
    assert dst.step == 0 and all(int(alg.optimizer.state[p]["step"]) == 24 for p in dev.parameters())
    after = dev.act(obs, seed=1, step=0)
    assert dev._bound_ptrs == ptrs                                               # no re-bind
    cpu = ref.clone(dev, torch.float32)
    np.testing.assert_allclose(after["mu"].cpu().numpy(), cpu.actor(obs.cpu()).detach().numpy(), rtol=ACT_RTOL, atol=ACT_ATOL)
    np.testing.assert_allclose(after["values"].cpu().numpy(), cpu.critic(obs.cpu()).detach().numpy(), rtol=ACT_RTOL, atol=ACT_ATOL)
    assert (after["mu"] - before["mu"]).abs().max() > 100 * ACT_ATOL and not torch.equal(after["sigma"], before["sigma"])


def test_checkpoints_load_into_the_other_backend(tmp_path):
    cfg = P.PPOConfig(num_steps_per_env=4, num_learning_epochs=1, num_mini_batches=2, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,))
    obs = _obs(50, seed=8)
    for first, second in (("hip", "torch"), ("torch", "hip")):
        trainer = P.PPOTrainer(_Standin(32, seed=1), cfg, seed=3, update=first)
        trainer.learn(2)
        path = str(tmp_path / f"{first}.pt")
        trainer.save(path)
        other = P.PPOTrainer(_Standin(32, seed=2), cfg, seed=4, update=second)
        other.load(path)
        sa, sb = trainer.alg.optimizer.state_dict(), other.alg.optimizer.state_dict()
        assert sa["state"].keys() == sb["state"].keys() and len(sa["state"]) == len(list(trainer.actor_critic.parameters()))
        assert all(float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) == 4.0 for k in sa["state"])
        assert all(torch.equal(sa["state"][k][m], sb["state"][k][m]) for k in sa["state"] for m in ("exp_avg", "exp_avg_sq"))
        assert torch.equal(other.get_inference_policy()(obs), trainer.get_inference_policy()(obs))
        assert other.alg.optimizer.param_groups[0]["lr"] == trainer.alg.optimizer.param_groups[0]["lr"]
        before = [p.detach().clone() for p in other.actor_critic.parameters()]
        infos = other.learn(1)                                                       # and training goes on from it
        assert other.iteration == 3 and all(np.isfinite(list(i.values())).all() for i in infos)
        assert all(float(s["step"]) == 6.0 for s in other.alg.optimizer.state_dict()["state"].values())
        assert all(not torch.equal(b, p) for b, p in zip(before, other.actor_critic.parameters()))


def test_learning_sanity_with_the_device_update():
    env = _Standin(256, seed=0)
    cfg = P.PPOConfig(num_steps_per_env=24, actor_hidden_dims=(64, 32), critic_hidden_dims=(64, 32), init_noise_std=0.5)
    trainer = P.PPOTrainer(env, cfg, seed=0, update="hip")
    policy = trainer.get_inference_policy()
    before = env.rms(policy)
    infos = trainer.learn(30)
    after = env.rms(policy)
    print(f"rms of clamp(mean) - c: {before:.3f} -> {after:.3f} (ratio {after / before:.2f}); mean reward {infos[0]['mean_reward']:.3f} -> {infos[-1]['mean_reward']:.3f}; "
          f"learning rate {infos[0]['learning_rate']:.3e} -> {infos[-1]['learning_rate']:.3e}")
    assert len(infos) == 30 and infos[-1]["iter"] == 30 and all(np.isfinite(list(i.values())).all() for i in infos)
    assert infos[-1]["learning_rate"] == trainer.alg.optimizer.param_groups[0]["lr"] == float(trainer.alg.lr_device)
    assert after <= 0.6 * before
