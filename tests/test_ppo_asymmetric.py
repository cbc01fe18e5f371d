"""The asymmetric actor-critic (privileged critic observations) without a GPU: the refusals of the new entry points of include/mpc_ppo.h and
include/mpc_ppo_update.h, the GEMM launches of mpc_ppo_update_grads when the two nets read rows of different widths (csrc/ppo_gemm_plan.h through
the shim of tests/test_ppo_gemm_plan.py), and the torch backend of rl_mpc_locomotion_amd.ppo with ``num_critic_obs``.

tests/ppo_asymmetric_ref.py wraps tests/ppo_update_ref.py for the critic's rows; the tolerances are those of tests/test_ppo.py's symmetric
counterpart (its own derivation: 1e-5 on the three loss terms, 1e-4 on the kl, whose terms cancel)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import ppo as P
from tests import ppo_asymmetric_ref as aref
from tests.test_ppo_gemm_plan import BACKWARD_DATA, BACKWARD_WEIGHT, FORWARD, plan  # noqa: F401  (the fixture)

E_ARG = -1
ints = lambda v: C.cast((C.c_int * len(v))(*v), C.c_void_p)


def test_refusals_come_back_before_the_device_is_touched():
    L = P.update_lib()
    err = L.mpc_ppo_last_error
    h = C.c_void_p()

    def create(a, c, na=None, nc=None):
        return L.mpc_ac_create_asymmetric(C.byref(h), len(a) - 1 if na is None else na, ints(a), len(c) - 1 if nc is None else nc, ints(c))
    good_a, good_c = [48, 32, 12], [64, 16, 1]
    assert L.mpc_ac_create_asymmetric(None, 2, ints(good_a), 2, ints(good_c)) == E_ARG and b"mpc_ac_create_asymmetric" in err()
    assert create([48, 32, 12], [60, 16, 1]) == E_ARG and b"multiples of 16" in err() and b"critic" in err()      # a width that is no multiple of 16
    assert create([40, 32, 12], good_c) == E_ARG and b"actor" in err() and create(good_a, [64, 24, 1]) == E_ARG
    assert create([48] + [16] * 8 + [12], good_c) == E_ARG and b"1 .. 8 layers" in err()                            # nine layers, either stack
    assert create(good_a, [64] + [16] * 8 + [1]) == E_ARG and create(good_a, good_c, na=0) == E_ARG and create(good_a, good_c, nc=0) == E_ARG
    assert create([48, 32, 8], good_c) == E_ARG and create(good_a, [64, 16, 2]) == E_ARG                            # not an actor / not a critic
    # more than 160 KiB of LDS on either net: 16 rows x (4096 + 4) + 16 x (16 + 4) words = 257 KiB for a 4096-wide first layer
    for a, c in (([4096, 16, 12], good_c), (good_a, [4096, 16, 1])):
        assert create(a, c) == E_ARG and b"LDS" in err()
    assert not h.value                                                       # nothing was created
    assert create([2048, 16, 12], good_c) == 0 and h.value                   # 129 KiB: the limit is on the wider net, and this one fits
    L.mpc_ac_destroy(h)
    h = C.c_void_p()
    # the plain creator keeps its refusal, with its own name in the text
    assert L.mpc_ac_create(C.byref(h), 2, ints(good_a), 2, ints(good_c)) == E_ARG and b"mpc_ac_create: actor and critic read the same observations" in err()
    p = 0x1000
    for a, c, equal in ((good_a, good_c, False), ([240, 32, 12], [16, 16, 1], False), ([48, 32, 12], [48, 16, 1], True)):
        assert create(a, c) == 0 and h.value
        rc = L.mpc_ac_act(h, 4, p, 1, 0, p, p, p, p, p, None, None)
        assert rc == E_ARG and ((b"bound" in err()) if equal else (b"mpc_ac_act_asymmetric" in err() and b"bound" not in err()))
        assert L.mpc_ac_act_asymmetric(h, 4, p, None, 1, 0, p, p, p, p, p, None, None) == E_ARG and b"d_critic_obs is null" in err()
        assert L.mpc_ac_act_asymmetric(h, 4, None, p, 1, 0, p, p, p, p, p, None, None) == E_ARG
        assert L.mpc_ac_act_asymmetric(h, 0, p, p, 1, 0, p, p, p, p, p, None, None) == E_ARG
        assert L.mpc_ac_act_asymmetric(h, 4, p, p, 1, 0, p + 4, p, p, p, p, None, None) == E_ARG and b"8-byte" in err()
        assert L.mpc_ac_act_asymmetric(h, 4, p, p, 1, 0, p, p, p, p, p, None, None) == E_ARG and b"bound" in err()      # all in order: nothing is bound
        assert L.mpc_ac_evaluate(h, 4, p, p, None) == E_ARG and L.mpc_ac_act_inference(h, 4, p, p, None) == E_ARG
        u = C.c_void_p()
        assert L.mpc_ppo_update_create(C.byref(u), h, 64) == E_ARG and b"bound" in err() and not u.value
        L.mpc_ac_destroy(h)
        h = C.c_void_p()
    assert L.mpc_ac_act_asymmetric(None, 4, p, p, 1, 0, p, p, p, p, p, None, None) == E_ARG
    # the critic's storage: a misaligned pointer is refused whatever the handle; a null handle too
    assert L.mpc_ppo_update_set_critic_storage(None, p + 4) == E_ARG and b"16-byte" in err()
    assert L.mpc_ppo_update_set_critic_storage(None, p) == E_ARG and b"16-byte" not in err()
    assert L.mpc_ppo_update_set_critic_storage(None, None) == E_ARG


def launches(actor, critic, rows):
    """mpc_ppo_update_grads' GEMM launches for dims lists actor = [width, hidden..., 12] and critic = [width, hidden..., 1], in its order, as
    tests/test_ppo_gemm_plan.launches restates them, but with a first width per net: (kind, actor's (M, N, K) or None, critic's).  Copied by hand from
    the forward and backward loops of csrc/mpc_ppo_update.hip, where layer 0 of net k reads its own rows with lda / ldb = dims[k][0]."""
    dims = [list(actor), list(critic)]
    nl = [len(d) - 1 for d in dims]
    out = []
    for l in range(max(nl)):
        out.append((FORWARD, *[(rows, d[l + 1], d[l]) if l < n else None for d, n in zip(dims, nl)]))
    for s in range(max(nl)):
        w, x = [], []
        for d, n in zip(dims, nl):
            l = n - 1 - s
            w.append((d[l + 1], d[l], rows) if l >= 0 else None)
            x.append((rows, d[l], d[l + 1]) if l > 0 else None)
        out.append((BACKWARD_WEIGHT, *w))
        if any(x):
            out.append((BACKWARD_DATA, *x))
    return out


@pytest.mark.parametrize("rows", (1, 33, 1040, 24576))
@pytest.mark.parametrize("actor, critic", (([240, 32, 12], [16, 32, 1]), ([16, 32, 12], [240, 32, 1])))
def test_the_plan_gives_each_net_its_own_first_layer(plan, actor, critic, rows):  # noqa: F811
    seq = launches(actor, critic, rows)
    assert [k for k, _, _ in seq] == [FORWARD, FORWARD, BACKWARD_WEIGHT, BACKWARD_DATA, BACKWARD_WEIGHT]
    # each net's layer-0 forward has its own K, each net's layer-0 backward weight its own N
    assert seq[0] == (FORWARD, (rows, 32, actor[0]), (rows, 32, critic[0])) and seq[0][1][2] != seq[0][2][2]
    assert seq[-1] == (BACKWARD_WEIGHT, (32, actor[0], rows), (32, critic[0], rows)) and seq[-1][1][1] != seq[-1][2][1]
    assert seq[3] == (BACKWARD_DATA, (rows, 32, 12), (rows, 32, 1))          # nothing flows into the observations: no data gradient at layer 0
    for kind, a, b in seq:
        p = plan(kind, a, b)
        bm, bn = 128, 128 if p["tile"] == "wide" else 64
        for shape, (tiles_m, tiles_n, chunks) in zip((a, b), p["problems"]):
            M, N, K = shape
            assert tiles_m * bm >= M > (tiles_m - 1) * bm and tiles_n * bn >= N > (tiles_n - 1) * bn      # the tiles cover this problem's own M x N
            if kind == BACKWARD_WEIGHT:
                assert chunks * p["chunk_rows"] >= K > (chunks - 1) * p["chunk_rows"]                    # and the chunks its rows
            else:
                assert chunks == 1
            assert p["grid_x"] >= tiles_m * tiles_n * chunks                  # the grid covers both problems
        assert p["grid_x"] == max(t[0] * t[1] * t[2] for t in p["problems"])
    # the wider net sets the grid of the first layer's weight gradient: 240 columns are four 64-wide tiles, 16 are one
    last = plan(*seq[-1])
    wide_net = 0 if actor[0] > critic[0] else 1
    assert last["tile"] == "narrow" and last["problems"][wide_net][1] == 4 and last["problems"][1 - wide_net][1] == 1


def test_the_critic_reads_its_own_rows_in_the_torch_path():
    torch.manual_seed(3)
    ac = P.ActorCritic(48, num_critic_obs=64, actor_hidden_dims=(32, 16), critic_hidden_dims=(16,))
    assert ac.num_obs == 48 and ac.num_critic_obs == ac.critic_width == 64
    assert ac.actor[0].weight.shape == (32, 48) and ac.critic[0].weight.shape == (16, 64)
    g = torch.Generator().manual_seed(4)
    obs, cobs, actions = torch.randn((9, 48), generator=g), torch.randn((9, 64), generator=g), torch.randn((9, 12), generator=g)
    logp, entropy, value, mu, sigma = ac.log_prob_entropy_value(obs, actions, cobs)
    assert torch.equal(value, ac.critic(cobs)) and torch.equal(mu, ac.actor(obs)) and value.shape == (9, 1)
    dist = torch.distributions.Normal(mu, mu * 0. + ac.std)
    assert torch.equal(logp, dist.log_prob(actions).sum(-1)) and torch.equal(entropy, dist.entropy().sum(-1)) and torch.equal(sigma, dist.stddev)
    other = ac.log_prob_entropy_value(obs, actions, cobs + 1.0)              # the critic's rows move the value and nothing else
    assert not torch.equal(other[2], value) and all(torch.equal(a, b) for a, b in zip(other[:2] + other[3:], (logp, entropy, mu, sigma)))
    with pytest.raises(RuntimeError):
        ac.log_prob_entropy_value(obs, actions)                             # 48 columns into a 64-wide critic: torch's own shape error
    with pytest.raises(ValueError, match="critic_obs"):
        ac.act(obs, 1, 0)                                                   # refused before the device is asked for


def test_the_symmetric_actor_critic_is_what_it_was():
    torch.manual_seed(1)
    a = P.ActorCritic(48)
    torch.manual_seed(1)
    b = P.ActorCritic(48, num_critic_obs=None)
    assert a.num_critic_obs is None and a.critic_width == 48
    want = {"std": (12,)}
    for net, dims in (("actor", (48, 512, 256, 128, 12)), ("critic", (48, 512, 256, 128, 1))):
        for i in range(4):
            want[f"{net}.{2 * i}.weight"] = (dims[i + 1], dims[i])
            want[f"{net}.{2 * i}.bias"] = (dims[i + 1],)
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == want and list(a.state_dict()) == list(b.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    wide = P.ActorCritic(48, num_critic_obs=240)                             # the same keys, one other shape
    assert list(wide.state_dict()) == list(a.state_dict())
    assert {k for k, v in wide.state_dict().items() if tuple(v.shape) != want[k]} == {"critic.0.weight"}
    st = P.RolloutStorage(4, 2, "cpu")
    assert st.privileged_observations is None and len(next(st.mini_batch_generator(1, 1))) == 8
    st = P.RolloutStorage(4, 2, "cpu", num_obs=48, num_privileged_obs=64)
    assert st.privileged_observations.shape == (2, 4, 64) and st.observations.shape == (2, 4, 48)
    batch = next(st.mini_batch_generator(1, 1))
    assert len(batch) == 9 and batch[8].shape == (8, 64)


def test_update_losses_match_a_float64_restatement():
    """tests/test_ppo.py::test_update_losses_match_a_float64_restatement with a 64-wide critic on rows of its own, to the same tolerances."""
    torch.manual_seed(5)
    cfg = P.PPOConfig(num_learning_epochs=1, num_mini_batches=1, actor_hidden_dims=(32, 16), critic_hidden_dims=(16,), init_noise_std=0.7)
    ac = P.ActorCritic(48, 12, cfg.actor_hidden_dims, cfg.critic_hidden_dims, cfg.init_noise_std, num_critic_obs=64)
    st = aref.filled_storage(ac, n=16, T=8, seed=6)
    st.step = st.T
    surrogate, value, entropy, kl, clipped_ratio, clipped_value = aref.losses64(ac, st, cfg.clip_param)
    assert 0.05 < clipped_ratio < 0.95 and 0.05 < clipped_value < 0.95          # both branches of both clips are taken
    shuffled = aref.losses64(ac, st, cfg.clip_param, critic_rows=st.privileged_observations.flip(1))
    assert abs(shuffled[1] - value) > 1e-3 * abs(value) and shuffled[0] == surrogate        # the restatement itself reads the critic's rows
    alg = P.PPO(ac, cfg)
    batch = next(st.mini_batch_generator(1, 1))
    got = [float(x.detach()) for x in alg.losses(batch)]
    want = aref.losses64(ac, st, cfg.clip_param, rows=batch_rows(st, batch))
    for g, w in zip(got[:3], want[:3]):
        assert abs(g - w) <= 1e-5 * abs(w), (g, w)
    assert abs(got[3] - want[3]) <= 1e-4 * abs(want[3]), (got[3], want[3])
    with pytest.raises(ValueError, match="critic rows"):
        alg.losses(batch[:8])
    before = [p.detach().clone() for p in ac.parameters()]
    mean_value, mean_surrogate = alg.update(st)
    got = [float(x) for x in alg.last_terms]
    print("update terms", got, "float64", (surrogate, value, entropy, kl))
    for g, w in zip(got[:3], (surrogate, value, entropy)):
        assert abs(g - w) <= 1e-5 * abs(w), (g, w)
    assert abs(got[3] - kl) <= 1e-4 * abs(kl), (got[3], kl)
    assert abs(float(mean_value) - value) <= 1e-5 * abs(value) and abs(float(mean_surrogate) - surrogate) <= 1e-5 * abs(surrogate)
    assert all(not torch.equal(b, p) for b, p in zip(before, ac.parameters())) and st.step == 0


def batch_rows(st, batch):
    """The storage rows a mini-batch holds, found by their (unique) observations."""
    flat = st.observations.flatten(0, 1)
    return [int((flat == row).all(1).nonzero()[0, 0]) for row in batch[0]]


def test_the_float64_wrapper_feeds_the_critic_its_rows():
    """tests/ppo_asymmetric_ref.py on top of tests/ppo_update_ref.py: with the critic's rows equal to the actor's it IS the symmetric reference."""
    from tests import ppo_update_ref as ref
    from tests.test_ppo import _filled_storage
    torch.manual_seed(5)
    cfg = P.PPOConfig(actor_hidden_dims=(32, 16), critic_hidden_dims=(16,), init_noise_std=0.7, num_mini_batches=1)
    sym = P.ActorCritic(48, 12, cfg.actor_hidden_dims, cfg.critic_hidden_dims, 0.7)
    st = _filled_storage(sym, n=8, T=4, seed=6)
    idx = torch.randperm(32, generator=torch.Generator().manual_seed(7))
    want = ref.grads_of(sym, cfg, st, idx, torch.float64)
    asym = P.ActorCritic(48, 12, cfg.actor_hidden_dims, cfg.critic_hidden_dims, 0.7, num_critic_obs=48)
    asym.load_state_dict(sym.state_dict())
    st2 = P.RolloutStorage(8, 4, "cpu", num_obs=48, num_privileged_obs=48)
    for f in ref.FIELDS:
        getattr(st2, f).copy_(getattr(st, f))
    st2.privileged_observations.copy_(st.observations)
    got = aref.grads_of(asym, cfg, st2, idx, torch.float64)
    assert all(torch.equal(a, b) for a, b in zip(got[0], want[0])) and got[1] == want[1] and got[2] == want[2]
    st2.privileged_observations.mul_(0.5)                                    # other rows for the critic: its gradients move, the actor's do not
    moved = aref.grads_of(asym, cfg, st2, idx, torch.float64)
    na = 2 * 3                                                               # actor weights and biases come first in mpc_ac_bind's order
    assert all(torch.equal(a, b) for a, b in zip(moved[0][:na], want[0][:na])) and all(not torch.equal(a, b) for a, b in zip(moved[0][na:-1], want[0][na:-1]))
    assert np.isfinite(moved[1]).all() and moved[1][1] != want[1][1] and moved[1][0] == want[1][0]


def test_fold_normalizer_folds_the_critic_statistics_into_the_critic():
    """obs_norm.fold_normalizer with the critic's own statistics: both folded nets on raw rows equal the nets on normalised rows (float64 on the
    host, so only the folded weights' one float32 rounding is left: 1e-5 of the output's size is generous for 64 terms)."""
    from rl_mpc_locomotion_amd.obs_norm import fold_normalizer
    torch.manual_seed(2)
    ac = P.ActorCritic(48, 12, (16,), (16,), num_critic_obs=64)
    g = torch.Generator().manual_seed(3)
    stats = lambda w: {"_mean": torch.randn((1, w), generator=g), "_std": torch.rand((1, w), generator=g) + 0.5}
    sa, sc = stats(48), stats(64)
    folded = P.ActorCritic(48, 12, (16,), (16,), num_critic_obs=64)
    folded.load_state_dict(fold_normalizer(ac.state_dict(), sa, eps=1e-2, critic_obs_norm_state_dict=sc))
    x, cx = torch.randn((9, 48), generator=g).double(), torch.randn((9, 64), generator=g).double()
    norm = lambda r, s: (r - s["_mean"].double()) / (s["_std"].double() + 1e-2)
    ac, folded = ac.double(), folded.double()
    for net, rows, s in (("actor", x, sa), ("critic", cx, sc)):
        want, got = getattr(ac, net)(norm(rows, s)).detach(), getattr(folded, net)(rows).detach()
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), net
    with pytest.raises(ValueError, match="64 observations"):
        fold_normalizer(ac.state_dict(), sa)                                # the actor's 48 statistics do not fit the 64-wide critic
