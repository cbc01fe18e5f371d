"""The collection half of a PPO iteration (csrc/ppo_rollout.h, include/mpc_ppo.h, rl_mpc_locomotion_amd.ppo) on the CPU: the header is compiled with
g++ into a small shim and driven through ctypes, against the torch restatement of rsl_rl in tests/ppo_ref.py; and the torch update.

Tolerances are derived, not measured from the code under test.  The time-out bootstrap, the GAE recursion and `returns - values` are chains of
correctly rounded float32 operations in a pinned order: bit-identical to the torch float32 loop.  `mean + std * eps` likewise.  The log-prob (torch's
own log and reduction order) and the normalised advantages (torch's own float32 mean and std) are held to 4 x torch's own float32-vs-float64 gap on
the same rows, which each test computes.  The sampler's bounds are five standard deviations of each statistic under the standard normal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, ppo as P
from tests import ppo_ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mpc_ppo.h")
HIPCC = "/opt/rocm/bin/hipcc"
GAMMA, LAM = 0.99, 0.95

SHIM = r"""
#include "ppo_rollout.h"
using namespace ppo;
extern "C" {
// out [n_env][n_step][12]
void shim_normals(unsigned long long seed, int env0, int n_env, int step0, int n_step, float *out) {
  for (int e = 0; e < n_env; ++e)
    for (int s = 0; s < n_step; ++s)
      for (int p = 0; p < kPairs; ++p) {
        float *o = out + ((long)e * n_step + s) * kActions + 2 * p;
        normal_pair(seed, env0 + e, step0 + s, p, o[0], o[1]);
      }
}
void shim_sample(unsigned long long seed, int n, int step, const float *mean, const float *std, float *eps, float *actions, float *logp) {
  for (int r = 0; r < n; ++r) logp[r] = sample_actions(seed, r, step, mean + 12 * r, std, eps + 12 * r, actions + 12 * r);
}
// the epilogue of the device kernel with the noise given
void shim_log_prob(int n, const float *mean, const float *std, const float *eps, float *actions, float *logp) {
  for (int r = 0; r < n; ++r) {
    float terms[kActions];
    for (int k = 0; k < kActions; ++k) {
      actions[12 * r + k] = action_of(mean[12 * r + k], std[k], eps[12 * r + k]);
      terms[k] = log_prob_term(actions[12 * r + k], mean[12 * r + k], std[k]);
    }
    logp[r] = log_prob_sum(terms);
  }
}
void shim_add(int n, float gamma, const float *rew, const long long *reset, const long long *timeout, const float *values, float *rewards, float *dones) {
  for (int r = 0; r < n; ++r) {
    rewards[r] = bootstrap(rew[r], gamma, values[r], timeout[r] != 0 ? 1.0f : 0.0f);
    dones[r] = reset[r] != 0 ? 1.0f : 0.0f;
  }
}
void shim_returns(int n, int T, float gamma, float lam, const float *rewards, const float *dones, const float *values, const float *last, float *returns,
                  float *raw, float *adv) {
  for (int r = 0; r < n; ++r) gae_column(T, n, rewards + r, dones + r, values + r, last[r], gamma, lam, returns + r, raw + r);
  double mean, std;
  moments(raw, (size_t)n * T, mean, std);
  for (long i = 0; i < (long)n * T; ++i) adv[i] = normalise_one(raw[i], mean, std);
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("ppo_shim")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    vp, ci, cf, u64 = C.c_void_p, C.c_int, C.c_float, C.c_ulonglong
    L.shim_normals.argtypes = [u64, ci, ci, ci, ci, vp]
    L.shim_sample.argtypes = [u64, ci, ci] + [vp] * 5
    L.shim_log_prob.argtypes = [ci] + [vp] * 5
    L.shim_add.argtypes = [ci, cf] + [vp] * 6
    L.shim_returns.argtypes = [ci, ci, cf, cf] + [vp] * 7
    for f in (L.shim_normals, L.shim_sample, L.shim_log_prob, L.shim_add, L.shim_returns):
        f.restype = None
    return L


def normals(L, seed, env0, n_env, step0, n_step):
    out = np.zeros((n_env, n_step, 12), np.float32)
    L.shim_normals(seed, env0, n_env, step0, n_step, out.ctypes.data)
    return out


def check_sampler_moments(eps):
    """eps [envs, steps, 12]: the bounds of the issue, each five standard deviations of its statistic for M standard normal draws."""
    x = eps.astype(np.float64)
    M = x.size
    assert np.isfinite(x).all()
    mean, var = x.mean(), x.var()
    tail = (np.abs(x) > 3).mean()
    p3 = 0.0027
    pair = np.corrcoef(x[..., 0::2].ravel(), x[..., 1::2].ravel())[0, 1]
    steps = np.corrcoef(x[:, :-1].ravel(), x[:, 1:].ravel())[0, 1]
    print(f"sampler: M {M} mean {mean:.3e} var-1 {var - 1:.3e} tail {tail:.5f} pair corr {pair:.3e} step corr {steps:.3e} max |eps| {np.abs(x).max():.3f}")
    assert abs(mean) < 5 / np.sqrt(M)
    assert abs(var - 1) < 5 * np.sqrt(2 / M)
    assert abs(tail - p3) < 5 * np.sqrt(p3 * (1 - p3) / M)
    assert abs(pair) < 5 / np.sqrt(M / 2) and abs(steps) < 5 / np.sqrt(M / 2)
    assert np.abs(x).max() <= 5.77                                               # sqrt(-2 log 2^-24) = 5.768: the documented truncation


def check_returns(rew_b, returns, raw, adv, rew, reset, time_outs, values, last, what):
    """Bootstrapped rewards, returns, un-normalised and normalised advantages [T,N] of the code under test against tests/ppo_ref.py on the same rows."""
    T, n = rew.shape
    dones = reset.to(torch.float32).unsqueeze(-1)
    want_b = torch.stack([ppo_ref.bootstrap(rew[t], values[t], time_outs[t], GAMMA) for t in range(T)])
    assert np.array_equal(rew_b, want_b.numpy()), f"{what}: bootstrapped rewards differ from the torch float32 loop"
    ret32, raw32, adv32 = ppo_ref.compute_returns(want_b.unsqueeze(-1), dones, values, last, GAMMA, LAM)
    assert np.array_equal(returns, ret32[..., 0].numpy()), f"{what}: returns differ from the torch float32 loop"
    assert np.array_equal(raw, raw32[..., 0].numpy()), f"{what}: returns - values differs from the torch float32 loop"
    if T * n < 2:
        assert np.isnan(adv).all() and torch.isnan(adv32).all()                  # torch's std of one value
        return
    adv64 = ppo_ref.normalise(raw32.double())                                    # the float64 evaluation on the same (bit-identical) rows
    gap = float((adv32.double() - adv64).abs().max())
    d = float(np.abs(adv.astype(np.float64) - adv32[..., 0].numpy()).max())
    print(f"{what}: normalised advantages off by {d:.3e} (bound {4 * gap:.3e})")
    assert gap > 0 and d <= 4 * gap, f"{what}: normalised advantages off by {d:.3e} > {4 * gap:.3e}"


def check_log_prob(actions, logp, mean, std, eps, what):
    """actions [n,12] and log-prob [n] of the code under test for the given mean, std, eps (numpy float32)."""
    m, s, e = torch.from_numpy(mean), torch.from_numpy(std), torch.from_numpy(eps)
    a32 = m + s * e
    assert np.array_equal(actions, a32.numpy()), f"{what}: actions differ from mean + std * eps in float32"
    lp32 = ppo_ref.log_prob(m, s, a32)
    lp64 = ppo_ref.log_prob(m.double(), s.double(), a32.double())
    gap = float((lp32.double() - lp64).abs().max())
    d = float(np.abs(logp.astype(np.float64) - lp32.numpy()).max())
    print(f"{what}: log-prob off by {d:.3e} (bound {4 * gap:.3e})")
    assert gap > 0 and d <= 4 * gap, f"{what}: log-prob off by {d:.3e} > {4 * gap:.3e}"


@pytest.mark.parametrize("T", (1, 2, 24))
def test_gae_matches_the_torch_loop(shim, T):
    n = 70
    rew, reset, time_outs, values, last = ppo_ref.rollout(T, n, seed=10 + T)
    assert reset[T - 1].any() and time_outs[0].any()
    if T == 24:
        assert 0.05 < reset.float().mean() < 0.25 and 0.02 < time_outs.float().mean() < 0.10
    a = lambda t, dt: np.ascontiguousarray(t.numpy(), dtype=dt)
    rew_b, dones = np.zeros((T, n), np.float32), np.zeros((T, n), np.float32)
    v = a(values[..., 0], np.float32)
    for t in range(T):
        shim.shim_add(n, GAMMA, a(rew[t], np.float32).ctypes.data, a(reset[t], np.int64).ctypes.data, a(time_outs[t], np.int64).ctypes.data, v[t].ctypes.data,
                      rew_b[t].ctypes.data, dones[t].ctypes.data)
    assert np.array_equal(dones, reset.numpy().astype(np.float32))
    returns, raw, adv = (np.zeros((T, n), np.float32) for _ in range(3))
    shim.shim_returns(n, T, GAMMA, LAM, rew_b.ctypes.data, dones.ctypes.data, v.ctypes.data, a(last[:, 0], np.float32).ctypes.data, returns.ctypes.data,
                      raw.ctypes.data, adv.ctypes.data)
    check_returns(rew_b, returns, raw, adv, rew, reset, time_outs, values, last, f"T = {T}")


def test_log_prob_matches_torch(shim):
    rng = np.random.default_rng(3)
    n = 64
    mean = rng.normal(0, 1, (n, 12)).astype(np.float32)
    std = rng.uniform(0.05, 2.0, 12).astype(np.float32)
    eps = rng.normal(0, 1, (n, 12)).astype(np.float32)
    actions, logp = np.zeros((n, 12), np.float32), np.zeros(n, np.float32)
    shim.shim_log_prob(n, mean.ctypes.data, std.ctypes.data, eps.ctypes.data, actions.ctypes.data, logp.ctypes.data)
    check_log_prob(actions, logp, mean, std, eps, "host")
    # sample_actions is the same epilogue behind the generator
    eps2, a2, lp2 = np.zeros((n, 12), np.float32), np.zeros((n, 12), np.float32), np.zeros(n, np.float32)
    shim.shim_sample(7, n, 3, mean.ctypes.data, std.ctypes.data, eps2.ctypes.data, a2.ctypes.data, lp2.ctypes.data)
    assert np.array_equal(eps2, normals(shim, 7, 0, n, 3, 1)[:, 0])
    check_log_prob(a2, lp2, mean, std, eps2, "host, own noise")


def test_sampler(shim):
    eps = normals(shim, 1, 0, 4096, 0, 16)                                       # M = 4096 * 12 * 16
    check_sampler_moments(eps)
    assert np.array_equal(normals(shim, 1, 5, 1, 0, 16)[0], eps[5])              # a draw does not change with the batch size
    assert np.array_equal(normals(shim, 1, 0, 80, 7, 1)[:, 0], eps[:80, 7])
    other = normals(shim, 2, 0, 64, 0, 16)
    assert not np.array_equal(other, eps[:64]) and abs(np.corrcoef(other.ravel(), eps[:64].ravel())[0, 1]) < 5 / np.sqrt(other.size)
    assert len(np.unique(eps)) > 0.99 * eps.size


def _filled_storage(ac, n, T, seed, zero_pad=0):
    """A CPU storage as a collection would leave it, from a slightly different (older) policy.  zero_pad: the last so many observation columns are
    exactly 0.0 in every row (the height scan's pad columns), and the policy's outputs are those of such rows."""
    g = torch.Generator().manual_seed(seed)
    st = P.RolloutStorage(n, T, "cpu", num_obs=ac.num_obs)
    r = lambda *shape: torch.randn(shape, generator=g)
    with torch.no_grad():
        st.observations.copy_(r(T, n, ac.num_obs))
        if zero_pad:
            st.observations[..., ac.num_obs - zero_pad:] = 0.0
        st.mu.copy_(ac.actor(st.observations) + 0.05 * r(T, n, 12))
        st.sigma.copy_((ac.std * (1.0 + 0.1 * torch.rand(12, generator=g))).expand(T, n, 12))
        st.actions.copy_(st.mu + st.sigma * r(T, n, 12))
        st.actions_log_prob.copy_(ppo_ref.log_prob(st.mu, st.sigma, st.actions).unsqueeze(-1))
        st.values.copy_(ac.critic(st.observations) + 0.3 * r(T, n, 1))
        st.returns.copy_(st.values + 0.5 * r(T, n, 1))
        st.advantages.copy_(0.5 + r(T, n, 1))
    return st


def _losses64(ac, st, clip):
    """The three loss terms and the kl of PPO.update's formulas in float64 numpy, over the whole storage as one mini-batch."""
    f = lambda t: t.detach().double().numpy().reshape(-1, t.shape[-1])

    def net(seq, x):
        for m in seq:
            x = x @ f(m.weight).T + m.bias.detach().double().numpy() if isinstance(m, torch.nn.Linear) else np.where(x > 0, x, np.expm1(x))
        return x
    obs, a, v_old, adv, ret, lp_old, mu_old, s_old = (f(t) for t in (st.observations, st.actions, st.values, st.advantages, st.returns, st.actions_log_prob,
                                                                      st.mu, st.sigma))
    mu, s, V = net(ac.actor, obs), ac.std.detach().double().numpy()[None, :], net(ac.critic, obs)
    logp = (-(a - mu) ** 2 / (2 * s ** 2) - np.log(s) - np.log(np.sqrt(2 * np.pi))).sum(-1)
    entropy = (0.5 + 0.5 * np.log(2 * np.pi) + np.log(s)).sum(-1) * np.ones(len(a))
    kl = (np.log(s / s_old + 1e-5) + (s_old ** 2 + (mu_old - mu) ** 2) / (2 * s ** 2) - 0.5).sum(-1).mean()
    ratio = np.exp(logp - lp_old[:, 0])
    A = adv[:, 0]
    surrogate = np.maximum(-A * ratio, -A * np.clip(ratio, 1 - clip, 1 + clip)).mean()
    value = np.maximum((V - ret) ** 2, (v_old + np.clip(V - v_old, -clip, clip) - ret) ** 2).mean()
    return surrogate, value, entropy.mean(), kl, (np.abs(ratio - 1) > clip).mean(), (np.abs(V - v_old) > clip).mean()


def test_update_losses_match_a_float64_restatement():
    torch.manual_seed(5)
    cfg = P.PPOConfig(num_learning_epochs=1, num_mini_batches=1, actor_hidden_dims=(32, 16), critic_hidden_dims=(16,), init_noise_std=0.7)
    ac = P.ActorCritic(48, 12, cfg.actor_hidden_dims, cfg.critic_hidden_dims, cfg.init_noise_std)
    st = _filled_storage(ac, n=16, T=8, seed=6)
    st.step = st.T
    surrogate, value, entropy, kl, clipped_ratio, clipped_value = _losses64(ac, st, cfg.clip_param)
    assert 0.05 < clipped_ratio < 0.95 and 0.05 < clipped_value < 0.95          # both branches of both clips are taken
    alg = P.PPO(ac, cfg)
    before = [p.detach().clone() for p in ac.parameters()]
    mean_value, mean_surrogate = alg.update(st)
    got = [float(x) for x in alg.last_terms]
    print("update terms", got, "float64", (surrogate, value, entropy, kl))
    for g, w in zip(got[:3], (surrogate, value, entropy)):
        assert abs(g - w) <= 1e-5 * abs(w), (g, w)
    # the kl's terms (about 0.5 each) cancel to about 0.006 per action: float32's 6e-8 becomes 5e-6 of the result, so it is held to 1e-4
    assert abs(got[3] - kl) <= 1e-4 * abs(kl), (got[3], kl)
    assert abs(float(mean_value) - value) <= 1e-5 * abs(value) and abs(float(mean_surrogate) - surrogate) <= 1e-5 * abs(surrogate)
    assert all(not torch.equal(b, p) for b, p in zip(before, ac.parameters())) and st.step == 0
    # mini-batches: T N // k rows each, every row at most once per epoch
    seen = [b[0].shape[0] for b in st.mini_batch_generator(3, 2)]
    assert seen == [16 * 8 // 3] * 6


def test_adaptive_schedule():
    ac = P.ActorCritic(48, 12, (16,), (16,))
    alg = P.PPO(ac, P.PPOConfig())
    lr0 = alg.learning_rate
    assert lr0 == 1e-3 and alg.cfg.desired_kl == 0.01
    lr = lambda: alg.optimizer.param_groups[0]["lr"]
    alg.adapt_learning_rate(0.021)                                               # > 2 desired_kl: down
    assert alg.learning_rate == lr() == lr0 / 1.5
    alg.adapt_learning_rate(0.0049)                                              # 0 < kl < desired_kl / 2: up
    assert alg.learning_rate == lr() == lr0 / 1.5 * 1.5
    here = alg.learning_rate
    for kl in (0.01, 0.005, 0.02, 0.0, -1e-9):                                   # in the band, on its edges, and not positive: unchanged
        alg.adapt_learning_rate(kl)
        assert alg.learning_rate == lr() == here
    for _ in range(40):
        alg.adapt_learning_rate(1.0)
    assert alg.learning_rate == lr() == 1e-5
    for _ in range(40):
        alg.adapt_learning_rate(1e-6)
    assert alg.learning_rate == lr() == 1e-2
    fixed = P.PPO(ac, P.PPOConfig(schedule="fixed", num_learning_epochs=1, num_mini_batches=1))
    st = _filled_storage(ac, n=4, T=4, seed=1)
    fixed.update(st)
    assert fixed.learning_rate == fixed.optimizer.param_groups[0]["lr"] == 1e-3


def test_state_dict_has_rsl_rl_keys_and_shapes():
    from rl_mpc_locomotion_amd import ActorCritic
    sd = ActorCritic().state_dict()
    want = {"std": (12,)}
    for net, dims in (("actor", (48, 512, 256, 128, 12)), ("critic", (48, 512, 256, 128, 1))):
        for i in range(4):
            want[f"{net}.{2 * i}.weight"] = (dims[i + 1], dims[i])
            want[f"{net}.{2 * i}.bias"] = (dims[i + 1],)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(sd)[0] == "std" and all(v.dtype == torch.float32 for v in sd.values())
    assert torch.equal(sd["std"], torch.ones(12)) and torch.equal(ActorCritic(init_noise_std=0.5).std.detach(), torch.full((12,), 0.5))
    assert all(isinstance(m, torch.nn.ELU) for m in list(ActorCritic().actor)[1::2])


def test_config_restates_the_reference():
    ref = "/root/reference/RL_Environment/tasks/legged_config_ppo.py"
    if not os.path.isfile(ref):
        pytest.skip("reference tree not present")
    ns = {}
    exec(compile(open(ref).read(), ref, "exec"), ns)
    R = ns["LeggedCfgPPO"]
    c = P.PPOConfig()
    assert c.seed == R.seed
    for k in ("init_noise_std", "activation"):
        assert getattr(c, k) == getattr(R.policy, k), k
    assert list(c.actor_hidden_dims) == R.policy.actor_hidden_dims and list(c.critic_hidden_dims) == R.policy.critic_hidden_dims
    for k in ("value_loss_coef", "use_clipped_value_loss", "clip_param", "entropy_coef", "num_learning_epochs", "num_mini_batches", "learning_rate", "schedule",
              "gamma", "lam", "desired_kl", "max_grad_norm"):
        assert getattr(c, k) == getattr(R.algorithm, k), k
    for k in ("num_steps_per_env", "max_iterations", "save_interval"):
        assert getattr(c, k) == getattr(R.runner, k), k


def test_abi_symbols_and_argument_checks():
    names = sorted(set(re.findall(r"\b(mpc_(?:ac|rollout|ppo)_[a-z_]+)\s*\(", open(HEADER).read())))
    assert names == sorted(P.SYMBOLS) and not set(names) & set(_lib.SYMBOLS)
    L = P.lib()
    for s in P.SYMBOLS:
        assert getattr(L, s).argtypes is not None, s
    E_ARG = -1
    ints = lambda v: C.cast((C.c_int * len(v))(*v), C.c_void_p)
    h = C.c_void_p()
    good_a, good_c = [48, 512, 256, 128, 12], [48, 64, 1]

    def create(a, c, na=None, nc=None):
        return L.mpc_ac_create(C.byref(h), len(a) - 1 if na is None else na, ints(a), len(c) - 1 if nc is None else nc, ints(c))
    assert L.mpc_ac_create(None, 4, ints(good_a), 2, ints(good_c)) == E_ARG
    assert create(good_a, good_c, na=0) == E_ARG and create(good_a, good_c, nc=0) == E_ARG                    # depths
    assert create([48] + [16] * 8 + [12], good_c) == E_ARG and create(good_a, [48] + [16] * 8 + [1]) == E_ARG  # nine layers
    assert create([48, 100, 12], good_c) == E_ARG and b"multiples of 16" in L.mpc_ppo_last_error()
    assert create([40, 64, 12], [40, 64, 1]) == E_ARG and create(good_a, [48, 24, 1]) == E_ARG
    assert create([48, 64, 17], good_c) == E_ARG and b"outputs" in L.mpc_ppo_last_error()
    assert create([48, 64, 8], good_c) == E_ARG and create(good_a, [48, 64, 2]) == E_ARG                     # not an actor / not a critic
    assert create(good_a, [64, 64, 1]) == E_ARG and b"same observations" in L.mpc_ppo_last_error()
    assert L.mpc_ac_create(C.byref(h), 4, None, 2, ints(good_c)) == E_ARG
    assert not h.value                                                           # nothing was created
    # a handle needs no device; binding validates the pointers before it looks for one
    assert create([48, 32, 12], [48, 16, 1]) == 0 and h.value
    ptrs = lambda v: C.cast((C.c_void_p * len(v))(*v), C.c_void_p)
    ok2 = ptrs([0x1000, 0x2000])
    assert L.mpc_ac_bind(None, ok2, ok2, ok2, ok2, 0x3000) == E_ARG
    assert L.mpc_ac_bind(h, None, ok2, ok2, ok2, 0x3000) == E_ARG
    assert L.mpc_ac_bind(h, ptrs([0x1000, 0]), ok2, ok2, ok2, 0x3000) == E_ARG and b"16-byte" in L.mpc_ppo_last_error()
    assert L.mpc_ac_bind(h, ok2, ptrs([0x1000, 0x2008]), ok2, ok2, 0x3000) == E_ARG
    assert L.mpc_ac_bind(h, ok2, ok2, ptrs([0x1004, 0x2000]), ok2, 0x3000) == E_ARG
    assert L.mpc_ac_bind(h, ok2, ok2, ok2, ok2, None) == E_ARG and L.mpc_ac_bind(h, ok2, ok2, ok2, ok2, 0x3004) == E_ARG
    # nothing bound: the launches refuse, again before any device call
    assert L.mpc_ac_act(h, 4, 0x1000, 1, 0, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None, None) == E_ARG and b"bound" in L.mpc_ppo_last_error()
    assert L.mpc_ac_evaluate(h, 4, 0x1000, 0x1000, None) == E_ARG and L.mpc_ac_act_inference(h, 4, 0x1000, 0x1000, None) == E_ARG
    assert L.mpc_ac_act(h, 0, 0x1000, 1, 0, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None, None) == E_ARG
    assert L.mpc_ac_act(h, 4, 0x1000, 1, 0, None, 0x1000, 0x1000, 0x1000, 0x1000, None, None) == E_ARG
    assert L.mpc_ac_act(h, 4, 0x1000, 1, 0, 0x1004, 0x1000, 0x1000, 0x1000, 0x1000, None, None) == E_ARG and b"8-byte" in L.mpc_ppo_last_error()
    assert L.mpc_ac_act(None, 4, 0x1000, 1, 0, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, None, None) == E_ARG
    L.mpc_ac_destroy(h)
    L.mpc_ac_destroy(None)
    p = 0x1000
    assert L.mpc_rollout_add(0, 0.99, p, p, p, p, p, p, None) == E_ARG and L.mpc_rollout_add(8, 0.99, p, None, p, p, p, p, None) == E_ARG
    assert L.mpc_rollout_add(8, 1.5, p, p, p, p, p, p, None) == E_ARG and L.mpc_rollout_add(8, float("nan"), p, p, p, p, p, p, None) == E_ARG
    assert L.mpc_rollout_returns(8, 0, 0.99, 0.95, p, p, p, p, p, p, None) == E_ARG and L.mpc_rollout_returns(0, 4, 0.99, 0.95, p, p, p, p, p, p, None) == E_ARG
    assert L.mpc_rollout_returns(8, 4, 0.99, 0.95, p, p, p, p, p, None, None) == E_ARG
    assert L.mpc_rollout_returns(8, 4, -0.1, 0.95, p, p, p, p, p, p, None) == E_ARG and L.mpc_rollout_returns(8, 4, 0.99, 2.0, p, p, p, p, p, p, None) == E_ARG


def test_classes_raise_without_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from rl_mpc_locomotion_amd import ActorCritic, PPOTrainer, RolloutStorage

    class Env:
        num_envs, num_obs, num_actions = 4, 48, 12
    with pytest.raises(_lib.MpcLibraryError):
        PPOTrainer(Env())
    ac = ActorCritic(48, 12, (16,), (16,))
    obs = torch.zeros((4, 48))
    for call in (lambda: ac.act(obs, 1, 0), lambda: ac.evaluate(obs), lambda: ac.act_inference(obs)):
        with pytest.raises(_lib.MpcLibraryError):
            call()
    st = RolloutStorage(4, 2, "cpu")
    with pytest.raises(_lib.MpcLibraryError):
        st.add(torch.zeros(4), torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long), 0.99)
    with pytest.raises(_lib.MpcLibraryError):
        st.compute_returns(torch.zeros((4, 1)), 0.99, 0.95)


def test_kernels_compile_for_gfx950_without_scratch(tmp_path):
    out = tmp_path / "mpc_ppo.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "mpc_ppo.hip"), "-o", str(out)], check=True, capture_output=True, text=True)
    remarks = r.stderr
    found = {}
    for name, scratch in re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", remarks, re.S):
        found[name] = int(scratch)
    for kernel in ("ac_kernel", "rollout_add_kernel", "returns_kernel", "normalise_kernel"):
        hit = [s for k, s in found.items() if kernel in k]
        assert hit == [0], (kernel, found)
