"""The device PPO update on the MI355X (include/mpc_ppo_update.h, rl_mpc_locomotion_amd.ppo.PPO(backend="hip")) against torch autograd +
torch.optim.Adam in float64 on the CPU (tests/ppo_update_ref.py), on the same storage, indices and hyper-parameters.

The tolerance is the project's rule: at most 4 x the distance of torch's own float32 run from the float64 run, which this module computes.  The
distance is pooled, because a single tensor's is one draw of a rounding error: gradients, parameter changes and moments are compared tensor by
tensor in relative L2, each held to 4 x the largest per-tensor gap over all row-count cases (and mini-batches, steps) of the same net pair; the
scalar terms as tests/test_ppo_update.py pools them, over the same cases.  Largest measured ratios error / gap: DESIGN.md section 8.3.

Those row counts all plan the 128 x 64 tile and 256-row weight-gradient chunks (csrc/ppo_gemm_plan.h).  BIG_ROWS x BIG_NETS are the cases that reach what
the training workload runs -- the 128 x 128 tile in all three kinds and chunks of 1024 and 512 rows -- with a pool of their own, so the cases above keep
their gaps; tests/test_ppo_gemm_plan.py pins which kernel each of this module's shapes reaches.

All of those rows are 48 columns wide.  WIDTHS x WIDE_NETS x WIDE_ROWS and BIG_WIDTHS are the same comparisons at other widths, each (net pair, width)
with a pool of its own: 16 (the narrowest row mpc_ac_create takes, half a reduction trip of the GEMM), 240 (the training row with the default height
scan: 48 task columns, 187 scan values and five pad columns that are exactly 0.0 in every row, as here) and 256 (where the first layer's weight
gradient takes the 128 x 128 tile).  At 16 385 rows a 240-wide first layer plans 1024-row chunks on the 128 x 64 tile with ldb = 240, which nothing else
does.  The gradient of a weight column whose input column is exactly zero is exactly zero, and Adam leaves such a column bit for bit where it was."""
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
# Net pairs for mpc_ppo_update_apply alone, by the number of float64 partials norm_kernel joins (tensors x ceil(largest numel / 4096)); its 1024 lanes
# take partials i, i + 1024, ..., and every pair above stays inside the first trip (the reference nets have the most: 17 x 32 = 544).
#   "second trip"  11 tensors x 128 blocks (the 512 x 1024 layer) = 1408: block 0 of both critic biases and of std lie at 1024, 1152 and 1280
#   "first past"   33 tensors (the most the ABI takes) x 32 blocks (512 x 256) = 1056: std's block 0 is partial 1024 itself, the first one of the second
#                  trip.  No pair has fewer partials with a live one past 1023: the last tensor's block 0 sits at (tensors - 1) x blocks, tensors is odd
#                  and at most 33, so blocks >= 32; 31 tensors would need 35 blocks (1085).
NORM_NETS = {"second trip": ((1024, 512), (64,)), "first past": ((512, 256, 16, 16, 16, 16, 16), (16,) * 7)}
NORM_PARTIALS = {"second trip": 1408, "first past": 1056}
ALL_NETS, ALL_ROWS = {**NETS, **BIG_NETS, **NORM_NETS}, {**ROWS, **BIG_ROWS}
DESIRED_KL = (0.01, 0.06, 1.0)                                                    # first-step kl 0.048 .. 0.076: down, unchanged, up
# Other widths than 48.  ZERO_PAD: width -> trailing columns that are exactly 0.0 in every row, as the height scan pads 48 + 187 to 240.
WIDTHS, WIDE_NETS, WIDE_ROWS = (16, 240), ("odd", "uneven"), ("chunked", "ragged")
BIG_WIDTHS = (240, 256)                                                            # on the reference nets at BIG_ROWS["production"]
ZERO_PAD = {240: 5}


def _cfg(nets, mini_batches=1, num_obs=48, **kw):
    """(PPOConfig carries no width: the nets take it from the task, here from _fixture's actor-critic; num_obs is accepted so a call names its case.)"""
    return P.PPOConfig(actor_hidden_dims=ALL_NETS[nets][0], critic_hidden_dims=ALL_NETS[nets][1], init_noise_std=0.7, num_mini_batches=mini_batches, **kw)


def _fixture(nets, rows, num_obs=48):
    """(CPU actor-critic, CPU storage, injected permutation) as tests/test_ppo.py builds them; the last ZERO_PAD[num_obs] observation columns zero."""
    n, T, mb = ALL_ROWS[rows]
    torch.manual_seed(5)
    ac = P.ActorCritic(num_obs, 12, *ALL_NETS[nets], init_noise_std=0.7)
    st = _filled_storage(ac, n=n, T=T, seed=6, zero_pad=ZERO_PAD.get(num_obs, 0))
    size = n * T // mb
    perm = torch.randperm(n * T, generator=torch.Generator().manual_seed(7))[:mb * size].contiguous()
    return ac, st, perm


def _to_device(ac, st, num_obs=None):
    dev = ref.clone(ac, torch.float32).to(DEV)
    out = P.RolloutStorage(st.n, st.T, DEV, num_obs=ac.num_obs if num_obs is None else num_obs)
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
    """Per net pair: float64 and float32 gradients and terms of every mini-batch of every row-count case, computed once.  At another width, over
    other row-count cases or with other settings of PPOConfig it is a pool of its own."""
    cache = {}

    def get(nets, num_obs=48, row_cases=tuple(ROWS), **cfg_kw):
        key = (nets, num_obs, row_cases, tuple(sorted(cfg_kw.items())))
        if key not in cache:
            cases = {}
            for rows in row_cases:
                ac, st, perm = _fixture(nets, rows, num_obs)
                mb = ROWS[rows][2]
                size = len(perm) // mb
                cfg = _cfg(nets, mb, num_obs, **cfg_kw)
                cases[rows] = [(ref.grads_of(ac, cfg, st, perm[i * size:(i + 1) * size], torch.float64),
                                ref.grads_of(ac, cfg, st, perm[i * size:(i + 1) * size], torch.float32)) for i in range(mb)]
            cache[key] = cases
        return cache[key]
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

    def get(nets, num_obs=48):
        if (nets, num_obs) not in cache:
            cases = {}
            for rows in BIG_ROWS:
                assert BIG_ROWS[rows][2] == 1
                ac, st, perm = _fixture(nets, rows, num_obs)
                cfg = _cfg(nets, 1, num_obs, desired_kl=0.06)
                cases[rows] = (ac, st, perm, ref.grads_of(ac, cfg, st, perm, torch.float64), ref.grads_of(ac, cfg, st, perm, torch.float32))
            cache[(nets, num_obs)] = cases
        return cache[(nets, num_obs)]
    return get


def _device_grads(alg, dst, perm, size, first=0):
    """One mpc_ppo_update_grads over rows first .. first + size of perm on alg's handle: (gradients, terms, learning rate) on the host."""
    L = P.update_lib()
    P.check(L.mpc_ppo_update_set_storage(alg._handle, dst.n * dst.T, *[getattr(dst, f).data_ptr() for f in ref.FIELDS]), "set_storage")
    idx = perm.to(DEV)
    terms = torch.zeros(4, device=DEV)
    alg.lr_device.fill_(1e-3)
    c = alg.cfg
    P.check(L.mpc_ppo_update_grads(alg._handle, size, idx.data_ptr() + 8 * first, c.clip_param, c.value_loss_coef, c.entropy_coef, int(c.use_clipped_value_loss), 1,
                                   c.desired_kl, alg.lr_device.data_ptr(), terms.data_ptr(), None), "grads")
    return [p.grad.cpu().clone() for p in alg.actor_critic.bind_order()], terms.cpu().clone(), float(alg.lr_device)


def _first_layer_weights(ac):
    names = _names(ac)
    return names.index("actor W0"), names.index("critic W0")


def _zero_pad_columns_are_exactly_zero(ac, grads, what):
    """The first-layer weight gradients of both nets: +0.0 or -0.0 bit for bit in the columns whose input is zero in every row, and some non-zero
    element in every other column."""
    live = ac.num_obs - ZERO_PAD[ac.num_obs]
    for k in _first_layer_weights(ac):
        g = grads[k]
        assert g.shape[1] == ac.num_obs and g.dtype == torch.float32
        assert bool(((g[:, live:].contiguous().view(torch.int32) & 0x7FFFFFFF) == 0).all()), f"{what}: {_names(ac)[k]} has a non-zero gradient in a column whose input is zero"
        assert bool((g[:, :live] != 0).any(0).all()), f"{what}: {_names(ac)[k]} has a live column without a gradient"


def _check_production(cases, nets, rows, what):
    """test_grads_match_float64_autograd's rule (desired_kl = 0.06) on one BIG_ROWS case of big_reference, the gaps pooled over `cases`."""
    gap = max(ref.rel_l2(g32, g64) for _, _, _, (g64s, _, _), (g32s, _, _) in cases.values() for g32, g64 in zip(g32s, g64s))
    rel = lambda x, r: abs(x - r) / abs(r)
    pool3 = max(rel(b[1][q], a[1][q]) for _, _, _, a, b in cases.values() for q in range(3))
    pool_kl = max(rel(b[1][3], a[1][3]) for _, _, _, a, b in cases.values())
    ac, st, perm, (g64s, t64, frac), _ = cases[rows]
    assert 0.05 < frac[0] < 0.95 and 0.05 < frac[1] < 0.95, frac
    dev, dst = _to_device(ac, st)
    alg = P.PPO(dev, _cfg(nets, 1, ac.num_obs, desired_kl=0.06), backend="hip")
    alg._device_state(len(perm))
    got, terms, lr = _device_grads(alg, dst, perm, len(perm))
    assert lr == ref.adapt(1e-3, t64[3], alg.cfg), t64[3]
    for q, name in enumerate(("surrogate", "value loss", "entropy", "kl")):
        g = pool_kl if q == 3 else pool3
        err = rel(float(terms[q]), t64[q])
        print(f"{what}: {name} off by {err:.3e} (bound {4 * g:.3e}, ratio {err / g:.3f})")
        assert g > 0 and err <= 4 * g, (name, err, g)
    names = _names(ac)
    for k in range(len(names)):
        print(f"{what}: {names[k]} off by {ref.rel_l2(got[k], g64s[k]):.3e}, its own float32 gap {ref.rel_l2(cases[rows][4][0][k], g64s[k]):.3e}")
    _pooled([(names[k], ref.rel_l2(got[k], g64s[k]), gap) for k in range(len(names))], f"{what}: gradients")
    return got


@pytest.mark.parametrize("rows", sorted(BIG_ROWS))
@pytest.mark.parametrize("nets", sorted(BIG_NETS))
def test_grads_on_the_production_plan_match_float64_autograd(big_reference, nets, rows):
    """test_grads_match_float64_autograd's rule (desired_kl = 0.06) at a row count that plans the wide tile and the long chunks; the float32 gap is
    pooled over the BIG_ROWS cases of this net pair only."""
    _check_production(big_reference(nets), nets, rows, f"{nets} {rows}")


@pytest.mark.parametrize("rows", sorted(BIG_ROWS))
@pytest.mark.parametrize("num_obs", BIG_WIDTHS)
def test_grads_on_the_production_plan_of_the_wide_rows_match_float64_autograd(big_reference, num_obs, rows):
    """The same at the widths training reaches with a height scan, on the reference nets, each width with a pool of its own.  At 240 columns and
    16 385 rows the first layer's weight gradient is the one launch that runs the 128 x 64 tile over 1024-row chunks (17, the last of one row), reads
    its rows through the index with ldb = 240 and ends in a column tile of 48 live columns; at 256 it takes the 128 x 128 tile
    (tests/test_ppo_gemm_plan.py pins both plans).  Measured error / gap: DESIGN.md section 8.3."""
    cases = big_reference("reference", num_obs)
    got = _check_production(cases, "reference", rows, f"reference {rows} at {num_obs} columns")
    if num_obs in ZERO_PAD:
        _zero_pad_columns_are_exactly_zero(cases[rows][0], got, f"reference {rows} at {num_obs} columns")


def _check_small(cases, nets, rows, num_obs=48, **cfg_kw):
    """test_grads_match_float64_autograd's rule on every mini-batch of one case of grads_reference, the gaps pooled over `cases`, under
    _cfg(nets, mini-batches, **cfg_kw); returns per mini-batch (device gradients, device terms, float64 terms, the bounds of the three loss terms and
    of the gradients)."""
    gap = max(ref.rel_l2(g32, g64) for case in cases.values() for (g64s, _, _), (g32s, _, _) in case for g32, g64 in zip(g32s, g64s))
    rel = lambda x, r: abs(x - r) / abs(r)
    pool3 = max(rel(b[1][q], a[1][q]) for case in cases.values() for a, b in case for q in range(3))
    pool_kl = max(rel(b[1][3], a[1][3]) for case in cases.values() for a, b in case)
    ac, st, perm = _fixture(nets, rows, num_obs)
    mb = ROWS[rows][2]
    size = len(perm) // mb
    dev, dst = _to_device(ac, st)
    alg = P.PPO(dev, _cfg(nets, mb, num_obs, **cfg_kw), backend="hip")
    alg._device_state(size)
    names, out = _names(ac), []
    for i in range(mb):
        what = f"{nets} {rows} at {num_obs} columns{''.join(f', {k} = {v}' for k, v in cfg_kw.items())}, mini-batch {i}"
        (g64s, t64, frac), _ = cases[rows][i]
        assert 0.05 < frac[0] < 0.95 and 0.05 < frac[1] < 0.95, frac
        got, terms, lr = _device_grads(alg, dst, perm, size, first=i * size)
        assert lr == ref.adapt(1e-3, t64[3], alg.cfg), t64[3]
        for q, name in enumerate(("surrogate", "value loss", "entropy", "kl")):
            g = pool_kl if q == 3 else pool3
            err = rel(float(terms[q]), t64[q])
            print(f"{what}: {name} off by {err:.3e} (bound {4 * g:.3e}, ratio {err / g:.3f})")
            assert g > 0 and err <= 4 * g, (name, err, g)
        _pooled([(names[k], ref.rel_l2(got[k], g64s[k]), gap) for k in range(len(names))], f"{what}: gradients")
        if num_obs in ZERO_PAD:
            _zero_pad_columns_are_exactly_zero(ac, got, what)
        out.append((got, terms, t64, 4 * pool3, 4 * gap))
    return out


@pytest.mark.parametrize("rows", WIDE_ROWS)
@pytest.mark.parametrize("num_obs", WIDTHS)
@pytest.mark.parametrize("nets", WIDE_NETS)
def test_grads_match_float64_autograd_at_other_widths(grads_reference, nets, num_obs, rows):
    """Every gradient tensor, the four terms and the learning-rate decision of every mini-batch at 16 and 240 columns, the float32 gap pooled over
    WIDE_ROWS of this net pair and width only."""
    _check_small(grads_reference(nets, num_obs, WIDE_ROWS), nets, rows, num_obs)


def test_the_unclipped_value_loss_matches_float64_autograd(grads_reference):
    """use_clipped_value_loss = 0 reaches head_row on the device: terms and gradients of the four ragged mini-batches against autograd under
    PPOConfig(use_clipped_value_loss=False), with a pool of their own; and the value loss is not the clipped run's, by more than the bound."""
    plain = _check_small(grads_reference("uneven", 48, ("ragged",), use_clipped_value_loss=False), "uneven", "ragged", use_clipped_value_loss=False)
    clipped = grads_reference("uneven")["ragged"]
    critic_w0 = _first_layer_weights(_fixture("uneven", "ragged")[0])[1]
    for i, (got, terms, t64, bound, grad_bound) in enumerate(plain):
        (c64s, c64, _), _ = clipped[i]
        assert all(abs(t64[q] - c64[q]) <= 1e-12 * abs(c64[q]) for q in (0, 2, 3))   # the flag moves the value loss alone
        away = abs(float(terms[1]) - c64[1]) / abs(c64[1])
        print(f"uneven ragged mini-batch {i}: value loss {float(terms[1]):.9g}, float64 unclipped {t64[1]:.9g}, float64 clipped {c64[1]:.9g}: {away:.3e} away (bound {bound:.3e})")
        assert away > bound and c64[1] > t64[1]
        assert ref.rel_l2(got[critic_w0], c64s[critic_w0]) > grad_bound                   # and the critic's gradient is not the clipped run's


def test_adam_leaves_the_weights_of_the_zero_columns_where_they_were():
    """One mpc_ppo_update_apply behind the 240-wide gradients: the first-layer weights that multiply the five zero columns are bit for bit what they
    were and their moments are zero; every tensor, and every other column of the two first-layer weights, moved."""
    nets, rows, num_obs = "uneven", "chunked", 240
    ac, st, perm = _fixture(nets, rows, num_obs)
    live = num_obs - ZERO_PAD[num_obs]
    dev, dst = _to_device(ac, st)
    alg = P.PPO(dev, _cfg(nets, 1, num_obs), backend="hip")
    alg._device_state(len(perm))
    grads, _, _ = _device_grads(alg, dst, perm, len(perm))
    _zero_pad_columns_are_exactly_zero(ac, grads, "before the step")
    params = dev.bind_order()
    before = [p.detach().cpu().clone() for p in params]
    P.check(P.update_lib().mpc_ppo_update_apply(alg._handle, alg.cfg.max_grad_norm, 0.9, 0.999, 1e-8, 1, alg.lr_device.data_ptr(), None), "apply")
    after = [p.detach().cpu() for p in params]
    assert all(not torch.equal(a, b) for a, b in zip(after, before))
    for k in _first_layer_weights(ac):
        assert torch.equal(after[k][:, live:].contiguous().view(torch.int32), before[k][:, live:].contiguous().view(torch.int32))
        assert bool((after[k][:, :live] != before[k][:, :live]).any(0).all())
        for key in ("exp_avg", "exp_avg_sq"):
            m = alg.optimizer.state[params[k]][key].cpu()
            assert bool((m[:, live:] == 0).all()) and bool((m[:, :live] != 0).any(0).all()), key


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


def test_a_larger_batch_on_a_used_handle_gets_a_handle_for_its_rows(grads_reference):
    """The 1040-row case on a PPO that has just run the 1-row case (rows > max_rows): the update handle is destroyed and created again for 1040 rows, its
    workspace with it.  Gradients, terms and learning rate are bit-identical to those of a PPO whose first handle was made for 1040 rows, and the gradients
    are within test_grads_match_float64_autograd's bound of float64 autograd."""
    nets = "uneven"
    cases = grads_reference(nets)
    gap = max(ref.rel_l2(g32, g64) for case in cases.values() for (g64s, _, _), (g32s, _, _) in case for g32, g64 in zip(g32s, g64s))
    one_ac, one_st, one_perm = _fixture(nets, "single")
    ac, st, perm = _fixture(nets, "chunked")
    assert all(torch.equal(a, b) for a, b in zip(ac.bind_order(), one_ac.bind_order()))         # the same nets with the same weights
    rows = len(perm)
    assert len(one_perm) == 1 and rows == 1040
    dev, dst = _to_device(ac, st)
    _, one_dst = _to_device(one_ac, one_st)
    grown = P.PPO(dev, _cfg(nets, 1), backend="hip")
    grown._device_state(1)
    assert grown._max_rows == 1
    _device_grads(grown, one_dst, one_perm, 1)
    grown._device_state(rows)
    assert grown._max_rows == rows                                                              # a new handle: the old one held one row
    a = _device_grads(grown, dst, perm, rows)
    fresh_dev, _ = _to_device(ac, st)
    fresh = P.PPO(fresh_dev, _cfg(nets, 1), backend="hip")
    fresh._device_state(rows)
    b = _device_grads(fresh, dst, perm, rows)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and a[2] == b[2]
    g64s = cases["chunked"][0][0][0]
    names = _names(ac)
    _pooled([(names[k], ref.rel_l2(a[0][k], g64s[k]), gap) for k in range(len(names))], "a handle recreated for more rows: gradients")


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
    _check_apply(ac, grads, runs, nets, max_norm)


def _check_apply(ac, grads, runs, nets, max_norm):
    """mpc_ppo_update_apply over the float32 gradients `grads` (one list per step) from ac's parameters: parameter changes and both moments after
    every step within 4 x the gap of runs[(m, float32)] from runs[(m, float64)] (ref.apply_steps), pooled over the steps, tensors and every m."""
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


@pytest.mark.parametrize("nets", sorted(NORM_NETS))
def test_apply_joins_more_norm_partials_than_one_trip_of_its_lanes(nets):
    """test_apply_matches_clip_and_adam's rule where norm_kernel's 1024 lanes walk their i += 1024 loop a second time (NORM_NETS).  The gradients are
    synthetic: normal draws scaled so that every tensor holds the same share of the squared norm, three different sets for the three steps, so the
    partials past 1023 (small tensors: biases and std) carry 3 / 11 and 1 / 33 of it and the clip at 0.25 depends on them."""
    torch.manual_seed(5)
    ac = P.ActorCritic(48, 12, *NORM_NETS[nets], init_noise_std=0.7)
    params = ac.bind_order()
    blocks = -(-max(p.numel() for p in params) // 4096)
    assert len(params) * blocks == NORM_PARTIALS[nets] > 1024                       # what mpc_ppo_update_apply hands to norm_kernel
    assert (len(params) - 1) * blocks >= 1024 and params[-1] is ac.std             # the last tensor's only live partial lies in the second trip
    g = torch.Generator().manual_seed(11)
    grads = [[torch.randn(p.shape, generator=g) / p.numel() ** 0.5 for p in params] for _ in range(3)]
    norms = [float(torch.cat([x.flatten() for x in gs]).double().norm()) for gs in grads]
    # tensor k's block b is partial k * blocks + b: what the second trip reads of it starts at block 1024 - k * blocks
    tail = [float(torch.cat([x.flatten()[4096 * max(0, 1024 - k * blocks):] for k, x in enumerate(gs)]).double().norm()) for gs in grads]
    print(f"{nets}: {len(params)} tensors x {blocks} blocks, norms {norms}, of which past partial 1023 {tail}")
    assert all(x > 1.0 for x in norms) and all(t > 0.1 * x for t, x in zip(tail, norms)), (norms, tail)      # 0.25 clips; the second trip is a tenth or more
    runs = {(0.25, dt): ref.apply_steps(ac, grads, 0.25, 1e-3 / 1.5, dt) for dt in (torch.float32, torch.float64)}
    _check_apply(ac, grads, runs, nets, 0.25)


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
