"""The asymmetric actor-critic on the MI355X: mpc_ac_act_asymmetric against the symmetric launch (the actor must not notice the critic), against
mpc_ac_evaluate and against torch; the device update with the critic's rows (mpc_ppo_update_set_critic_storage) against float64 autograd fed those
rows (tests/ppo_asymmetric_ref.py); and PPOTrainer on a task with a height scan, observation noise and privileged observations.

Tolerances are the symmetric tests' own: tests/test_ppo_gpu.py's value comparison (ACT_RTOL / ACT_ATOL of tests/test_policy.py) and the rule of
tests/test_ppo_update_gpu.py -- at most 4 x the distance of torch's own float32 run from the float64 run, pooled per net pair over the row-count
cases, tensor by tensor in relative L2 and term by term as there."""
import numpy as np
import pytest
import torch

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, curriculum as K, domain_rand as D, height_scan as HS, ppo as P, privileged_obs as V, rl_task as R
from tests import ppo_asymmetric_ref as aref
from tests import ppo_update_ref as ref
from tests.test_height_scan_gpu import TROT, _cfg, _robots, _yaw, grid
from tests.test_policy import ACT_ATOL, ACT_RTOL
from tests.test_ppo_update_gpu import ROWS as SYMMETRIC_ROWS, _names, _pooled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (actor width, critic width): the wider net is the other one in each, so both orders of the LDS sizing and both grids of the first layer run
PAIRS = {"wide critic": (48, 64), "wide actor": (240, 16)}
HIDDEN = ((32,), (16,))
# mini-batch rows -> (n, T) of the storage they are drawn from; 1040 is the count tests/test_ppo_update_gpu.py crosses the 256-row chunks with
CASES = {1: (3, 2), 33: (7, 6), 1040: SYMMETRIC_ROWS["chunked"][:2]}
assert SYMMETRIC_ROWS["chunked"] == (65, 16, 1)


def _net(pair, seed=1, symmetric=False):
    """A random actor-critic on the CPU: biases of size 0.1 and std in [0.05, 2] as tests/test_ppo_gpu.py draws them."""
    a0, c0 = PAIRS[pair]
    torch.manual_seed(seed)
    ac = P.ActorCritic(a0, 12, *HIDDEN, num_critic_obs=None if symmetric else c0)
    with torch.no_grad():
        ac.std.copy_(torch.rand(12) * 1.95 + 0.05)
        for p in ac.parameters():
            if p.dim() == 1 and p is not ac.std:
                p.copy_(torch.randn_like(p) * 0.1)
    return ac


def _rows(n, w, seed):
    return (torch.randn((n, w), generator=torch.Generator().manual_seed(seed)) * 1.5).to(DEV)


@pytest.mark.parametrize("n", (1, 17))
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_act_asymmetric(pair, n):
    a0, c0 = PAIRS[pair]
    cpu = _net(pair)
    dev = aref.clone(cpu, torch.float32).to(DEV)
    sym = _net(pair, seed=2, symmetric=True)                                 # another critic (a0 wide), the same actor and std
    sym.load_state_dict({k: v for k, v in cpu.state_dict().items() if not k.startswith("critic")}, strict=False)
    sym = sym.to(DEV)
    obs, cobs = _rows(n, a0, seed=10 + n), _rows(n, c0, seed=20 + n)
    out = dev.act(obs, seed=3, step=n, return_eps=True, critic_obs=cobs)
    plain = sym.act(obs, seed=3, step=n, return_eps=True)
    for k in ("actions", "actions_log_prob", "mu", "sigma", "eps"):          # the actor does not notice the critic
        assert torch.equal(out[k], plain[k]), k
    assert out["values"].shape == (n, 1) and torch.equal(out["values"], dev.evaluate(cobs))
    assert torch.equal(dev.act_inference(obs), out["mu"])
    want = cpu.double().critic(cobs.cpu().double()).detach().numpy()
    np.testing.assert_allclose(out["values"].cpu().numpy(), want, rtol=ACT_RTOL, atol=ACT_ATOL)
    assert not torch.equal(out["values"], plain["values"])
    # written into a storage's slot, as the trainer does, the same bits
    st = P.RolloutStorage(n, 2, DEV, num_obs=a0, num_privileged_obs=c0)
    dev.act(obs, seed=3, step=n, out=st.slot(1), critic_obs=cobs)
    assert torch.equal(st.values[1], out["values"]) and torch.equal(st.actions[1], out["actions"]) and float(st.values[0].abs().max()) == 0
    # the plain launch is refused on unequal widths, and the tensors are checked at each net's own width
    with pytest.raises(ValueError, match="critic_obs"):
        dev.act(obs, seed=3, step=n)
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*mpc_ac_act_asymmetric"):
        P.check(P.lib().mpc_ac_act(dev._handle, n, obs.data_ptr(), 3, n, *[out[k].data_ptr() for k in ("actions", "actions_log_prob", "values", "mu", "sigma")],
                                   None, None), "mpc_ac_act")
    with pytest.raises(ValueError):
        dev.act(obs, seed=3, step=n, critic_obs=obs if a0 != c0 else cobs[:, :-1])
    with pytest.raises(ValueError):
        dev.evaluate(obs)


def _fixture(pair, rows):
    """(CPU actor-critic, CPU storage with rows of their own for the critic, the mini-batch's indices: a repeated row and the storage's last row
    among them)."""
    n, T = CASES[rows]
    ac = _net(pair, seed=5)
    with torch.no_grad():
        ac.std.fill_(0.7)
    st = aref.filled_storage(ac, n=n, T=T, seed=6)
    idx = torch.randperm(n * T, generator=torch.Generator().manual_seed(7))[:rows].contiguous()
    idx[-1] = n * T - 1
    if rows > 1:
        idx[1] = idx[0]
        assert len(set(idx.tolist())) < rows
    assert int(idx.max()) == n * T - 1 and len(idx) == rows <= n * T
    return ac, st, idx


def _cfg_ppo(**kw):
    return P.PPOConfig(actor_hidden_dims=HIDDEN[0], critic_hidden_dims=HIDDEN[1], init_noise_std=0.7, num_mini_batches=1, **kw)


@pytest.fixture(scope="module")
def reference():
    """Per width pair: for every row-count case the float64 and float32 runs of one mini-batch and of the Adam step behind it, computed once."""
    cache = {}

    def get(pair):
        if pair not in cache:
            cfg, cases = _cfg_ppo(), {}
            for rows in CASES:
                ac, st, idx = _fixture(pair, rows)
                runs = {}
                for dt in (torch.float64, torch.float32):
                    grads, terms, frac = aref.grads_of(ac, cfg, st, idx, dt)
                    lr = ref.adapt(1e-3, terms[3], cfg)
                    runs[dt] = (grads, terms, frac, lr, aref.apply_step(ac, grads, cfg.max_grad_norm, lr, dt))
                assert runs[torch.float32][3] == runs[torch.float64][3]      # torch's own two runs decide alike: the steps are comparable
                cases[rows] = runs
            cache[pair] = cases
        return cache[pair]
    return get


def _to_device(ac, st):
    dev = aref.clone(ac, torch.float32).to(DEV)
    out = P.RolloutStorage(st.n, st.T, DEV, num_obs=ac.num_obs, num_privileged_obs=ac.critic_width if st.privileged_observations is not None else None)
    for f in (aref.FIELDS if st.privileged_observations is not None else ref.FIELDS):
        getattr(out, f).copy_(getattr(st, f))
    out.step = out.T
    return dev, out


def _device_step(dev, dst, idx, critic_rows="own"):
    """mpc_ppo_update_grads over `idx` and one mpc_ppo_update_apply on a fresh handle: (gradients, terms, learning rate, parameters after the step).
    critic_rows: "own" = the storage's privileged rows, None = no call at all (a symmetric run), or a tensor."""
    alg = P.PPO(dev, _cfg_ppo(), backend="hip")
    size = len(idx)
    alg._device_state(size)
    L = P.update_lib()
    P.check(L.mpc_ppo_update_set_storage(alg._handle, dst.n * dst.T, *[getattr(dst, f).data_ptr() for f in ref.FIELDS]), "set_storage")
    if critic_rows is not None:
        rows = dst.privileged_observations if isinstance(critic_rows, str) else critic_rows
        P.check(L.mpc_ppo_update_set_critic_storage(alg._handle, rows.data_ptr()), "set_critic_storage")
    d_idx, terms, c = idx.to(DEV), torch.zeros(4, device=DEV), alg.cfg
    alg.lr_device.fill_(1e-3)
    P.check(L.mpc_ppo_update_grads(alg._handle, size, d_idx.data_ptr(), c.clip_param, c.value_loss_coef, c.entropy_coef, int(c.use_clipped_value_loss), 1,
                                   c.desired_kl, alg.lr_device.data_ptr(), terms.data_ptr(), None), "grads")
    grads = [p.grad.cpu().clone() for p in dev.bind_order()]
    P.check(L.mpc_ppo_update_apply(alg._handle, c.max_grad_norm, 0.9, 0.999, 1e-8, 1, alg.lr_device.data_ptr(), None), "apply")
    return grads, terms.cpu().clone(), float(alg.lr_device), [p.detach().cpu().clone() for p in dev.bind_order()], alg


@pytest.mark.parametrize("rows", sorted(CASES))
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_update_matches_float64_autograd_fed_the_critic_rows(reference, pair, rows):
    cases = reference(pair)
    rel = lambda x, r: abs(x - r) / abs(r)
    gap = max(ref.rel_l2(g32, g64) for c in cases.values() for g32, g64 in zip(c[torch.float32][0], c[torch.float64][0]))
    pool3 = max(rel(c[torch.float32][1][q], c[torch.float64][1][q]) for c in cases.values() for q in range(3))
    pool_kl = max(rel(c[torch.float32][1][3], c[torch.float64][1][3]) for c in cases.values())
    ac, st, idx = _fixture(pair, rows)
    p0 = [p.detach().double() for p in ac.bind_order()]
    step_gap = max(ref.rel_l2(a.double() - p, b - p) for c in cases.values() for a, b, p in zip(c[torch.float32][4], c[torch.float64][4], p0))
    g64s, t64, frac, lr64, p64 = cases[rows][torch.float64]
    if rows > 1:
        assert 0.05 < frac[0] < 0.95 and 0.05 < frac[1] < 0.95, frac
    dev, dst = _to_device(ac, st)
    grads, terms, lr, params, _ = _device_step(dev, dst, idx)
    what = f"{pair} {rows} rows"
    assert lr == lr64, (lr, lr64, t64[3])
    for q, name in enumerate(("surrogate", "value loss", "entropy", "kl")):
        g = pool_kl if q == 3 else pool3
        err = rel(float(terms[q]), t64[q])
        print(f"{what}: {name} off by {err:.3e} (bound {4 * g:.3e}, ratio {err / g:.3f})")
        assert g > 0 and err <= 4 * g, (name, err, g)
    names = _names(ac)
    a0, c0 = PAIRS[pair]
    assert grads[names.index("actor W0")].shape == (32, a0) and grads[names.index("critic W0")].shape == (16, c0)
    _pooled([(names[k], ref.rel_l2(grads[k], g64s[k]), gap) for k in range(len(names))], f"{what}: gradients")
    _pooled([(names[k], ref.rel_l2(params[k].double() - p0[k], p64[k] - p0[k]), step_gap) for k in range(len(names))], f"{what}: parameter change")
    if rows > 1:                                                             # (one row may sit in a clipped branch, whose gradient is zero)
        assert all(not torch.equal(a.double(), b) for a, b in zip(params, p0))
    # a rerun on a fresh handle and fresh copies is bit-identical
    dev2, dst2 = _to_device(ac, st)
    again = _device_step(dev2, dst2, idx)
    assert all(torch.equal(a, b) for a, b in zip(grads, again[0])) and torch.equal(terms, again[1]) and lr == again[2]
    assert all(torch.equal(a, b) for a, b in zip(params, again[3]))
    # the critic's rows are what moves the critic: with other rows its gradients differ, the actor's do not
    dev3, dst3 = _to_device(ac, st)
    other = _device_step(dev3, dst3, idx, critic_rows=(dst3.privileged_observations * 0.5).contiguous())
    na = 2 * len(ac._linears(ac.actor))
    assert all(torch.equal(a, b) for a, b in zip(grads[:na], other[0][:na])) and torch.equal(grads[-1], other[0][-1])
    if rows > 1:
        assert all(not torch.equal(a, b) for a, b in zip(grads[na:-1], other[0][na:-1]))


@pytest.mark.parametrize("rows", sorted(CASES))
def test_aliased_to_the_actor_rows_the_update_is_the_symmetric_one(rows):
    """Equal widths, the critic's storage pointing at the actor's rows: bit for bit the symmetric path's gradients, terms, rate and parameters."""
    n, T = CASES[rows]
    torch.manual_seed(5)
    sym = P.ActorCritic(48, 12, *HIDDEN, init_noise_std=0.7)
    from tests.test_ppo import _filled_storage
    st = _filled_storage(sym, n=n, T=T, seed=6)
    idx = torch.randperm(n * T, generator=torch.Generator().manual_seed(7))[:rows].contiguous()
    idx[-1] = n * T - 1
    want = _device_step(*_to_device(sym, st), idx, critic_rows=None)
    asym = P.ActorCritic(48, 12, *HIDDEN, init_noise_std=0.7, num_critic_obs=48)
    asym.load_state_dict(sym.state_dict())
    dev, dst = _to_device(asym, st)
    assert dst.privileged_observations is None
    got = _device_step(dev, dst, idx, critic_rows=dst.observations)
    assert all(torch.equal(a, b) for a, b in zip(got[0], want[0])) and torch.equal(got[1], want[1]) and got[2] == want[2]
    assert all(torch.equal(a, b) for a, b in zip(got[3], want[3])) and all(float(g.abs().max()) > 0 for g in got[0])
    # and a symmetric handle takes the pointer too, and gives it back (NULL clears it)
    dev2, dst2 = _to_device(sym, st)
    both = _device_step(dev2, dst2, idx, critic_rows=dst2.observations)
    assert all(torch.equal(a, b) for a, b in zip(both[0], want[0]))
    # an asymmetric handle without the critic's rows is refused before anything is launched
    dev3, dst3 = _to_device(asym, st)
    with pytest.raises(_lib.MpcLibraryError, match=r"\(-1\).*mpc_ppo_update_set_critic_storage"):
        _device_step(dev3, dst3, idx, critic_rows=None)
    alg = got[4]
    P.check(P.update_lib().mpc_ppo_update_set_critic_storage(alg._handle, None), "clear")
    terms = torch.zeros(4, device=DEV)
    assert P.update_lib().mpc_ppo_update_grads(alg._handle, rows, idx.to(DEV).data_ptr(), 0.2, 1.0, 0.01, 1, 0, 0.0, None, terms.data_ptr(), None) == -1


def test_the_python_update_passes_the_critic_rows():
    """PPO.update(backend="hip") on a storage with privileged rows: the same parameters as the hand-made calls above, chained over two epochs."""
    pair, rows = "wide critic", 33
    ac, st, _ = _fixture(pair, rows)
    n, T = CASES[rows]
    perm = torch.randperm(n * T, generator=torch.Generator().manual_seed(9))[:2 * (n * T // 2)].contiguous()
    cfg = P.PPOConfig(actor_hidden_dims=HIDDEN[0], critic_hidden_dims=HIDDEN[1], init_noise_std=0.7, num_mini_batches=2, num_learning_epochs=2)
    outs = []
    for _ in range(2):
        dev, dst = _to_device(ac, st)
        alg = P.PPO(dev, cfg, backend="hip")
        alg.update(dst, indices=perm.to(DEV))
        assert len(alg._storage_ptrs) == 9 and alg._storage_ptrs[8] == dst.privileged_observations.data_ptr()
        outs.append([p.detach().cpu().clone() for p in dev.bind_order()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    # against the float64 loop of tests/ppo_update_ref.py's update, restated for the critic's rows: the first mini-batch's step alone is compared
    # above; here it is enough that the critic moved and that a storage without the rows is refused
    assert all(not torch.equal(a, b.detach()) for a, b in zip(outs[0], ac.bind_order()))
    dev, dst = _to_device(ac, st)
    dst.privileged_observations = None
    with pytest.raises(_lib.MpcLibraryError, match="set_critic_storage"):
        P.PPO(dev, cfg, backend="hip").update(dst, indices=perm.to(DEV))


class _Recording:
    """The task with every privileged row it hands out kept (a clone on the device), at the reset and after every step."""

    def __init__(self, env):
        self.env, self.seen = env, []
        self.num_envs, self.num_obs, self.num_actions, self.device, self.cfg = env.num_envs, env.num_obs, env.num_actions, env.device, env.cfg
        self.num_privileged_obs, self.progress_buf = env.num_privileged_obs, env.progress_buf

    @property
    def privileged_obs_buf(self):
        return self.env.privileged_obs_buf

    def reset(self):
        obs = self.env.reset()
        self.seen.append(self.env.privileged_obs_buf.clone())
        return obs

    def step(self, actions):
        out = self.env.step(actions)
        self.seen.append(self.env.privileged_obs_buf.clone())
        return out


N_ENVS, STEPS = 64, 4


def _task(privileged=True):
    g = grid()
    cfg = _cfg(episode_length_s=0.05, seed=4)
    scan = HS.HeightScan(N_ENVS, device=DEV)
    dr = D.DomainRand(N_ENVS, observations=D.NoiseSpec.legged_gym(cfg, height_scan=scan), seed=3, device=DEV)
    origin = g.tile_origins.reshape(-1, 2)[np.arange(N_ENVS) % 6]
    return R.BatchedRLTask(_robots(N_ENVS), [TROT] * N_ENVS, cfg=cfg, device=DEV, yaw0=_yaw(N_ENVS), terrain=g.terrain, origin=origin, height_scan=scan,
                           domain_rand=dr, privileged_obs=V.PrivilegedObs(N_ENVS, device=DEV) if privileged else None)


def _pcfg():
    return P.PPOConfig(num_steps_per_env=STEPS, num_learning_epochs=1, num_mini_batches=2, actor_hidden_dims=(64, 32), critic_hidden_dims=(32,), init_noise_std=0.5)


def _finite(infos):
    flat = []
    for i in infos:
        for v in i.values():
            flat += list(v.values()) if isinstance(v, dict) else list(np.ravel(v))
    return bool(np.isfinite(np.asarray(flat, dtype=np.float64)).all())


@pytest.mark.parametrize("update", ("torch", "hip"))
def test_trainer_with_privileged_observations(update, tmp_path):
    task = _task()
    wp = task.num_privileged_obs
    assert wp == 240 == task.num_obs                                         # 48 + 187 + 5 both: the same width, other columns
    env = _Recording(task)
    trainer = P.PPOTrainer(env, _pcfg(), seed=3, update=update)
    ac, st = trainer.actor_critic, trainer.storage
    assert ac.num_critic_obs == wp and ac.critic[0].weight.shape == (32, wp) and ac.actor[0].weight.shape == (64, 240)
    assert st.privileged_observations.shape == (STEPS, N_ENVS, wp) and trainer.critic_obs_norm is None
    trainer.collect()
    seen = torch.stack(env.seen)                                             # the reset's row and the STEPS ticks'
    assert seen.shape == (STEPS + 1, N_ENVS, wp)
    assert torch.equal(st.privileged_observations, seen[:STEPS])             # slot t: the rows the values of slot t were computed from
    assert torch.equal(trainer.critic_obs, seen[STEPS]) and trainer.critic_obs.data_ptr() == task.privileged_obs_buf.data_ptr()
    assert torch.equal(st.values[1], ac.evaluate(st.privileged_observations[1].contiguous()))
    assert torch.equal(trainer.last_values, ac.evaluate(seen[STEPS]))
    # the critic's rows are the clean ones: they differ from the actor's noisy rows in the live columns, and their tail is contacts and phase
    assert not torch.equal(st.privileged_observations[..., :235], st.observations[..., :235])
    assert bool(((st.privileged_observations[..., 235:239] == 0) | (st.privileged_observations[..., 235:239] == 1)).all())
    assert (st.observations[..., 235:] == 0).all().item() and float(st.privileged_observations[..., 239].max()) > 0
    before = [p.detach().clone() for p in ac.parameters()]
    infos = trainer.learn(2)
    assert len(infos) == 2 and _finite(infos)
    assert all(not torch.equal(a, b) for a, b in zip(before, ac.parameters()))
    path = str(tmp_path / "ck.pt")
    trainer.save(path)
    ck = torch.load(path)
    assert "critic_obs_norm_state_dict" not in ck and ck["model_state_dict"]["critic.0.weight"].shape == (32, wp)
    # a trainer on a task without the option is what it was; and it refuses this checkpoint by naming both widths
    plain = P.PPOTrainer(_task(privileged=False), _pcfg(), seed=3, update=update)
    assert plain.storage.privileged_observations is None and plain.num_privileged_obs is None and plain.actor_critic.num_critic_obs is None
    plain.learn(1)
    assert plain.critic_obs is None and len(plain.alg._storage_ptrs or ()) in (0, 8)
    narrow = P.PPOTrainer(_Narrow(task), _pcfg(), seed=3, update=update)
    with pytest.raises(ValueError, match="240 columns.*64"):
        narrow.load(path)


class _Narrow:
    """Stands for an environment whose critic rows are 64 wide (never stepped)."""

    def __init__(self, env):
        self.num_envs, self.num_obs, self.num_actions, self.device, self.num_privileged_obs = env.num_envs, env.num_obs, env.num_actions, env.device, 64


def test_save_load_learn_reproduces_a_straight_run_on_the_device_update(tmp_path):
    straight = P.PPOTrainer(_task(), _pcfg(), seed=3, update="hip")
    straight.learn(3)
    resumed = P.PPOTrainer(_task(), _pcfg(), seed=3, update="hip")
    resumed.learn(2)
    path = str(tmp_path / "ck.pt")
    resumed.save(path)
    resumed.load(path)
    resumed.learn(1)
    assert resumed.iteration == straight.iteration == 3
    for (k, a), b in zip(straight.actor_critic.state_dict().items(), resumed.actor_critic.state_dict().values()):
        assert torch.equal(a, b), k
    assert straight.infos == resumed.infos
    sa, sb = straight.alg.optimizer.state_dict()["state"], resumed.alg.optimizer.state_dict()["state"]
    assert all(torch.equal(sa[k][m], sb[k][m]) for k in sa for m in ("exp_avg", "exp_avg_sq"))


def test_trainer_normalises_the_critic_rows_with_statistics_of_their_own(tmp_path):
    task = _task()
    trainer = P.PPOTrainer(task, _pcfg(), seed=3, update="hip", normalize_obs=True)
    assert trainer.critic_obs_norm is not None and trainer.critic_obs_norm.num_obs == 240 and trainer.critic_obs_norm is not trainer.obs_norm
    infos = trainer.learn(2)
    assert _finite(infos)
    path = str(tmp_path / "ck.pt")
    trainer.save(path)
    ck = torch.load(path)
    rows = N_ENVS * (2 * STEPS + 1)                                          # the reset's rows and every tick's, once each
    assert int(ck["critic_obs_norm_state_dict"]["count"]) == int(ck["obs_norm_state_dict"]["count"]) == rows
    assert not torch.equal(ck["critic_obs_norm_state_dict"]["_mean"], ck["obs_norm_state_dict"]["_mean"])
    st = trainer.storage
    assert torch.isfinite(st.privileged_observations).all().item()
    assert not torch.equal(trainer.critic_obs, task.privileged_obs_buf)      # the normalised copy
    other = P.PPOTrainer(_task(), _pcfg(), seed=4, update="hip", normalize_obs=True)
    other.load(path)
    assert torch.equal(other.critic_obs_norm.state64, trainer.critic_obs_norm.state64) and int(other.critic_obs_norm.count) == rows
    other.learn(1)
    assert _finite(other.infos)
