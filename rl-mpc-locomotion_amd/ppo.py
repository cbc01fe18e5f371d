"""PPO training of the weight policy: device rollouts, GAE, trainer (include/mpc_ppo.h, csrc/mpc_ppo.hip, csrc/ppo_rollout.h).

The reference trains through rsl_rl's ``OnPolicyRunner`` (RL_Environment/train.py:61-81, hyper-parameters in
RL_Environment/tasks/legged_config_ppo.py); rsl_rl itself is an empty submodule there.  This module restates rsl_rl v1.0.2's
``ActorCritic``, ``RolloutStorage``, ``PPO`` and runner by their published formulas, split where the work splits:

* the **collection half** of an iteration runs once per environment tick and is HIP: ``ActorCritic.act`` is one launch (actor and critic
  side by side, sampling and log-prob in the actor's epilogue) that writes straight into slot t of the storage, ``RolloutStorage.add`` is
  one kernel (time-out bootstrap and done flag, read from the task's int64 buffers), ``compute_returns`` is two (GAE, normalisation).
  The kernels read the torch parameters where the optimiser updates them in place: no weight copy is made, ever.
* the **update half** (``PPO.update``: mini-batch Adam steps) is GEMMs with autograd and is plain torch by default, on whatever device the
  storage lives on; ``PPO(..., backend="hip")`` / ``PPOTrainer(..., update="hip")`` select the device update (include/mpc_ppo_update.h,
  csrc/mpc_ppo_update.hip, csrc/ppo_gemm.h, csrc/ppo_update.h): forward and backward GEMMs on the fp32 MFMA pipe, the loss head, the gradient
  clip and Adam, on the parameters, ``.grad`` tensors and optimiser moments where torch keeps them, with no host read per mini-batch.

    env = BatchedRLTask(robot_type, gait_id)
    trainer = PPOTrainer(env)
    trainer.learn(num_iterations)
    trainer.save("model.pt")
    policy = WeightPolicy.from_state_dict(torch.load("model.pt")["model_state_dict"])

Not rsl_rl's: the exploration noise is a counter-based generator keyed by (seed, environment, step, action pair), not torch's, so parity
with ``Normal.sample`` is in distribution only, and |eps| <= 5.768 (ppo_rollout.h).  Opt-in, each described where ``PPOTrainer`` takes it: observation
normalisation (rsl_rl 2.x's ``EmpiricalNormalization``; ``obs_norm.ObsNormalizer``), privileged critic observations (rsl_rl's ``num_critic_obs``; the
reference uses none), recurrent policies (rsl_rl's ``ActorCriticRecurrent``: an LSTM in front of each MLP; ``recurrent.py``), the runner's episode
statistics on the device (``episode.EpisodeStats``); ``PPOTrainer.evaluate`` is the reference's ``cfg.test`` loop.  Not built: GRU and stacked layers,
logging beyond ``infos``.  (A recurrent actor-critic's device update is ``RecurrentConfig(update_through_time="hip", update_heads="hip")``; a recurrent
``update="hip"`` stays refused.)  Teacher-student policy distillation -- a teacher whose actor reads the privileged row, a student that is labelled with its
actions, PPO fine-tuning of the student -- is ``distill.py`` (``TeacherEnv``, ``Distiller``), with nothing changed here.

The device entry points need the GPU (MpcLibraryError without one) and have no CPU fallback.
"""
import ctypes as C
from collections import namedtuple
from dataclasses import dataclass
from itertools import islice

import torch
from torch import nn

from . import _lib
from ._lib import cd, ci, ll, need_gpu, pvp, tensor_arg, text, vp
from .episode import S_EPISODES, S_MEAN_LENGTH, S_MEAN_RETURN, S_WINDOW_COUNT, S_WINDOW_TIMEOUTS, EpisodeStats, random_progress
from .obs_norm import ObsNormalizer

NUM_ACTIONS = 12

# the entry points of include/mpc_ppo.h (bound here, not in _lib.SYMBOLS, which lists include/mpc_batch.h)
DECLS = {
    "mpc_ac_create": (ci, [pvp, ci, vp, ci, vp]),
    "mpc_ac_create_asymmetric": (ci, [pvp, ci, vp, ci, vp]),
    "mpc_ac_destroy": (None, [vp]),
    "mpc_ac_bind": (ci, [vp, vp, vp, vp, vp, vp]),
    "mpc_ac_act": (ci, [vp, ci, vp, C.c_ulonglong, C.c_uint, vp, vp, vp, vp, vp, vp, vp]),
    "mpc_ac_act_asymmetric": (ci, [vp, ci, vp, vp, C.c_ulonglong, C.c_uint, vp, vp, vp, vp, vp, vp, vp]),
    "mpc_ac_evaluate": (ci, [vp, ci, vp, vp, vp]),
    "mpc_ac_act_inference": (ci, [vp, ci, vp, vp, vp]),
    "mpc_ac_act_distill": (ci, [vp, vp, ci, vp, vp, C.c_ulonglong, C.c_uint, vp, vp, vp, vp, vp, vp]),
    "mpc_rollout_add": (ci, [ci, cd, vp, vp, vp, vp, vp, vp, vp]),
    "mpc_rollout_returns": (ci, [ci, ci, cd, cd, vp, vp, vp, vp, vp, vp, vp]),
    "mpc_ppo_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS)                           # libmpc_batch.so with the PPO entry points bound
check = _lib.checker(lib, "mpc_ppo_last_error")

# the entry points of include/mpc_ppo_update.h, with a binding of their own
UPDATE_DECLS = {
    "mpc_ppo_update_create": (ci, [pvp, vp, ci]),
    "mpc_ppo_update_destroy": (None, [vp]),
    "mpc_ppo_update_tensors": (ci, [vp]),
    "mpc_ppo_update_workspace_bytes": (ll, [vp]),
    "mpc_ppo_update_layer_gradient": (ci, [vp, ci, ci, pvp, vp]),
    "mpc_ppo_update_bind": (ci, [vp, vp, vp, vp]),
    "mpc_ppo_update_set_storage": (ci, [vp, ll] + [vp] * 8),
    "mpc_ppo_update_set_critic_storage": (ci, [vp, vp]),
    "mpc_ppo_update_grads": (ci, [vp, ci, vp, cd, cd, cd, ci, ci, cd, vp, vp, vp]),
    "mpc_ppo_update_apply": (ci, [vp, cd, cd, cd, cd, ci, vp, vp]),
    "mpc_ppo_update_set_sequence_rows": (ci, [vp, vp, vp, vp, vp]),
    "mpc_ppo_update_grads_sequence": (ci, [vp, ci, vp, cd, cd, cd, ci, ci, cd, vp, vp, vp]),
    "mpc_ppo_update_bind_extra": (ci, [vp, ci, vp, vp, vp, vp, vp]),
    "mpc_ppo_update_set_distill_targets": (ci, [vp, vp]),
    "mpc_ppo_update_grads_distill": (ci, [vp, ci, vp, ci, vp, vp]),
    "mpc_ppo_update_apply_actor": (ci, [vp, cd, cd, cd, cd, ci, vp, vp]),
}
UPDATE_SYMBOLS = list(UPDATE_DECLS)
update_lib = _lib.binder(UPDATE_DECLS, base=lib)   # ... with the entry points of the device update bound (and those of ``lib()``)


@dataclass
class PPOConfig:
    """``LeggedCfgPPO`` (RL_Environment/tasks/legged_config_ppo.py) restated as numbers."""
    seed: int = 1                                  # :2
    # policy
    init_noise_std: float = 1.0                    # :5
    actor_hidden_dims: tuple = (512, 256, 128)     # :6
    critic_hidden_dims: tuple = (512, 256, 128)    # :7
    activation: str = "elu"                        # :8  (the only one built)
    # algorithm
    value_loss_coef: float = 1.0                   # :12
    use_clipped_value_loss: bool = True            # :13
    clip_param: float = 0.2                        # :14
    entropy_coef: float = 0.01                     # :15
    num_learning_epochs: int = 5                   # :16
    num_mini_batches: int = 4                      # :17  mini-batch size = num_envs * num_steps_per_env / num_mini_batches
    learning_rate: float = 1.0e-3                  # :18
    schedule: str = "adaptive"                     # :19  'adaptive' or 'fixed'
    gamma: float = 0.99                            # :20
    lam: float = 0.95                              # :21
    desired_kl: float = 0.01                       # :22
    max_grad_norm: float = 1.0                     # :23
    # runner
    num_steps_per_env: int = 24                    # :28  per iteration
    max_iterations: int = 5000                     # :29
    save_interval: int = 100                       # :32


def mlp(num_in, hidden, num_out):
    layers, d = [], num_in
    for h in hidden:
        layers += [nn.Linear(d, h), nn.ELU()]
        d = h
    layers.append(nn.Linear(d, num_out))
    return nn.Sequential(*layers)


class ActorCritic(nn.Module):
    """rsl_rl's ``ActorCritic`` with ELU: ``actor`` and ``critic`` are ``nn.Sequential`` stacks of Linear / ELU, ``std`` is the
    state-independent action noise, so ``state_dict()`` has rsl_rl's keys (``std``, ``actor.{0,2,..}.{weight,bias}``,
    ``critic.{0,2,..}.{weight,bias}``) and loads through ``WeightPolicy.from_state_dict``.

    ``act``, ``evaluate`` and ``act_inference`` run the device kernels on the parameters where they are (no gradient flows through
    them); ``log_prob_entropy_value`` is the differentiable torch path of the update.

    ``num_critic_obs`` (rsl_rl's; None: the critic reads the actor's rows, as before): the critic's first ``Linear`` has that width and the critic's
    rows are an argument of their own -- ``act(obs, ..., critic_obs=)``, ``evaluate(critic_obs)``, ``log_prob_entropy_value(obs, actions, critic_obs)``
    -- through the asymmetric entry points (``mpc_ac_create_asymmetric``, ``mpc_ac_act_asymmetric``).  The state dict has the same keys either way.

    The call form is ``ActorCriticRecurrent``'s, one for both: ``hidden_sizes`` (None here) is what a ``RolloutStorage`` keeps per slot,
    ``reset_memory()`` does nothing, ``reset=`` / ``saved=`` must be None (ValueError otherwise)."""
    hidden_sizes = None

    def __init__(self, num_obs=48, num_actions=NUM_ACTIONS, actor_hidden_dims=(512, 256, 128), critic_hidden_dims=(512, 256, 128), init_noise_std=1.0,
                 num_critic_obs=None):
        super().__init__()
        if num_actions != NUM_ACTIONS:
            raise ValueError("the sampling kernel draws six Box-Muller pairs: twelve actions (the MPC weights)")
        self.num_obs, self.num_actions = int(num_obs), int(num_actions)
        self.num_critic_obs = None if num_critic_obs is None else int(num_critic_obs)
        self.critic_width = self.num_obs if num_critic_obs is None else self.num_critic_obs      # what the critic's first layer reads
        self.actor = mlp(num_obs, actor_hidden_dims, num_actions)
        self.critic = mlp(self.critic_width, critic_hidden_dims, 1)
        self.std = nn.Parameter(init_noise_std * torch.ones(num_actions))
        self._handle, self._bound_ptrs = None, None

    __del__ = _lib.finalizer("mpc_ac_destroy")

    # ---- the device path -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _linears(seq):
        return [m for m in seq if isinstance(m, nn.Linear)]

    def _ready(self, what, obs, width=None, critic_obs=None):
        """The handle, bound to the parameters' current device addresses (checked on every call: ``.to()`` moves them, an optimiser step
        or ``load_state_dict`` does not).  ``obs`` has ``width`` columns (None: ``num_obs``); ``critic_obs``, when given, ``critic_width``."""
        need_gpu(what, obs, self.std)
        if critic_obs is not None:
            need_gpu(what, critic_obs)
        la, lc = self._linears(self.actor), self._linears(self.critic)
        if self._handle is None:
            dims = lambda ls: [ls[0].in_features] + [m.out_features for m in ls]
            h = C.c_void_p()
            create = "mpc_ac_create" if self.num_critic_obs is None else "mpc_ac_create_asymmetric"
            check(getattr(lib(), create)(C.byref(h), len(la), _lib.int_array(dims(la)), len(lc), _lib.int_array(dims(lc))), create)
            self._handle = h
        ptrs = _lib.addresses_to_bind(self.bind_order(), self._bound_ptrs, self.std.device, "ActorCritic parameters must be contiguous float32 tensors on one device")
        if ptrs is not None:
            na, nc, arr = len(la), len(lc), _lib.ptr_array
            with torch.cuda.device(self.std.device):
                check(lib().mpc_ac_bind(self._handle, arr(ptrs[:na]), arr(ptrs[na:2 * na]), arr(ptrs[2 * na:2 * na + nc]),
                                        arr(ptrs[2 * na + nc:2 * na + 2 * nc]), ptrs[-1]), "mpc_ac_bind")
            self._bound_ptrs = ptrs
        n = obs.shape[0]
        tensor_arg(obs, torch.float32, n * (self.num_obs if width is None else width), "obs")
        if critic_obs is not None:
            tensor_arg(critic_obs, torch.float32, n * self.critic_width, "critic_obs")
        return n

    def bind_order(self):
        """The parameters in ``mpc_ac_bind``'s order: actor weights, actor biases, critic weights, critic biases, std."""
        la, lc = self._linears(self.actor), self._linears(self.critic)
        return [m.weight for m in la] + [m.bias for m in la] + [m.weight for m in lc] + [m.bias for m in lc] + [self.std]

    def reset_memory(self):
        pass

    @staticmethod
    def _no_memory(what, *given):
        if any(x is not None for x in given):
            raise ValueError(f"{what}: reset= / saved= on a feed-forward actor-critic, which has no memory")

    def act(self, obs, seed, step, out=None, return_eps=False, critic_obs=None, reset=None, saved=None):
        """``ActorCritic.act`` + ``evaluate`` in one launch: obs [n, num_obs] -> a dict of ``actions`` [n,12], ``actions_log_prob`` [n,1],
        ``values`` [n,1], ``mu`` [n,12], ``sigma`` [n,12] (and ``eps`` [n,12] if asked).  ``out``: the same dict of caller's tensors to write
        into (slot t of a RolloutStorage: ``storage.slot(t)``).  The noise of environment r is a function of (seed, r, step) alone.
        ``critic_obs`` [n, critic_width]: the rows the critic reads (required when ``num_critic_obs`` was given); still one launch."""
        self._no_memory("ActorCritic.act", reset, saved)
        if critic_obs is None and self.num_critic_obs is not None:
            raise ValueError("this actor-critic was made with num_critic_obs: act needs critic_obs")
        n = self._ready("ActorCritic.act", obs, critic_obs=critic_obs)
        dev = obs.device
        if out is None:
            e = lambda k: torch.empty((n, k), dtype=torch.float32, device=dev)
            out = dict(actions=e(12), actions_log_prob=e(1), values=e(1), mu=e(12), sigma=e(12))
        else:
            for k, w in (("actions", 12), ("actions_log_prob", 1), ("values", 1), ("mu", 12), ("sigma", 12)):
                tensor_arg(out[k], torch.float32, n * w, k)
        eps = torch.empty((n, 12), dtype=torch.float32, device=dev) if return_eps else None
        tail = (int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, out["actions"].data_ptr(), out["actions_log_prob"].data_ptr(), out["values"].data_ptr(),
                out["mu"].data_ptr(), out["sigma"].data_ptr(), eps.data_ptr() if return_eps else None, _lib.stream(dev))
        if critic_obs is None:
            check(lib().mpc_ac_act(self._handle, n, obs.data_ptr(), *tail), "mpc_ac_act")
        else:
            check(lib().mpc_ac_act_asymmetric(self._handle, n, obs.data_ptr(), critic_obs.data_ptr(), *tail), "mpc_ac_act_asymmetric")
        if return_eps:
            out = dict(out, eps=eps)
        return out

    def evaluate(self, obs, out=None, reset=None):
        """The critic alone: obs [n, critic_width] (the critic's own rows when ``num_critic_obs`` was given) -> values [n, 1]."""
        self._no_memory("ActorCritic.evaluate", reset)
        n = self._ready("ActorCritic.evaluate", obs, width=self.critic_width)
        values = torch.empty((n, 1), dtype=torch.float32, device=obs.device) if out is None else tensor_arg(out, torch.float32, n, "out")
        check(lib().mpc_ac_evaluate(self._handle, n, obs.data_ptr(), values.data_ptr(), _lib.stream(obs.device)), "mpc_ac_evaluate")
        return values

    def act_inference(self, obs, reset=None):
        """The actor's mean: obs [n, num_obs] -> [n, 12], bit for bit the raw action of ``WeightPolicy.step`` on the same weights."""
        self._no_memory("ActorCritic.act_inference", reset)
        n = self._ready("ActorCritic.act_inference", obs)
        mean = torch.empty((n, 12), dtype=torch.float32, device=obs.device)
        check(lib().mpc_ac_act_inference(self._handle, n, obs.data_ptr(), mean.data_ptr(), _lib.stream(obs.device)), "mpc_ac_act_inference")
        return mean

    # ---- the differentiable path of the update ---------------------------------------------------------------------------------------------
    def log_prob_entropy_value(self, obs, actions, critic_obs=None):
        """(log-prob [B], entropy [B], value [B,1], mu [B,12], sigma [B,12]) of ``actions`` under the current parameters, in plain torch with
        autograd: ``Normal(actor(obs), std)`` as rsl_rl's ``update_distribution`` builds it; the value is the critic's of ``critic_obs`` (None: of
        ``obs``, rsl_rl's ``critic_obs = privileged_obs if privileged_obs is not None else obs``)."""
        mu = self.actor(obs)
        dist = torch.distributions.Normal(mu, mu * 0. + self.std)
        return dist.log_prob(actions).sum(dim=-1), dist.entropy().sum(dim=-1), self.critic(obs if critic_obs is None else critic_obs), mu, dist.stddev


class RolloutStorage:
    """rsl_rl's ``RolloutStorage`` without its staging: [T, N, ...] float32 tensors ``observations`` [T,N,num_obs], ``actions``, ``mu``,
    ``sigma`` [T,N,12], ``values``, ``rewards``, ``dones``, ``actions_log_prob``, ``returns``, ``advantages`` [T,N,1].  ``ActorCritic.act``
    writes into ``slot(t)``; ``add`` and ``compute_returns`` are device kernels (a storage on the CPU can be filled by hand and read by
    ``PPO.update``, which is plain torch).  ``num_privileged_obs`` (rsl_rl's; None: no such tensor): ``privileged_observations`` [T,N,Wp], the
    critic's rows, which the mini-batch generator then yields last.  ``hidden`` = (H_a, H_c) (None: no such tensors): ``saved_h_a``, ``saved_c_a``
    [T,N,H_a] and ``saved_h_c``, ``saved_c_c`` [T,N,H_c], the state each memory of a recurrent actor-critic started slot t from (written by the cell
    launch through ``hidden_slot(t)``), which ``recurrent_mini_batch_generator`` reads."""

    def __init__(self, n, T, device, num_obs=48, num_actions=NUM_ACTIONS, num_privileged_obs=None, hidden=None):
        self.n, self.T, self.device = int(n), int(T), torch.device(device)
        z = lambda k: torch.zeros((self.T, self.n, k), dtype=torch.float32, device=self.device)
        self.observations, self.actions, self.mu, self.sigma = z(num_obs), z(num_actions), z(num_actions), z(num_actions)
        self.values, self.rewards, self.dones, self.actions_log_prob, self.returns, self.advantages = z(1), z(1), z(1), z(1), z(1), z(1)
        self.privileged_observations = None if num_privileged_obs is None else z(int(num_privileged_obs))
        self.hidden = None if hidden is None else (int(hidden[0]), int(hidden[1]))
        if self.hidden is not None:
            self.saved_h_a, self.saved_c_a, self.saved_h_c, self.saved_c_c = z(self.hidden[0]), z(self.hidden[0]), z(self.hidden[1]), z(self.hidden[1])
        self.step = 0

    def slot(self, t):
        """The views of slot t that ``ActorCritic.act(..., out=)`` writes."""
        return dict(actions=self.actions[t], actions_log_prob=self.actions_log_prob[t], values=self.values[t], mu=self.mu[t], sigma=self.sigma[t])

    def hidden_slot(self, t):
        """The views of slot t that ``ActorCriticRecurrent.act(..., saved=)`` writes: the state the memories started the slot from (None: none are kept)."""
        return None if self.hidden is None else dict(h_a=self.saved_h_a[t], c_a=self.saved_c_a[t], h_c=self.saved_h_c[t], c_c=self.saved_c_c[t])

    def add(self, rew, reset, time_outs, gamma, obs=None):
        """``PPO.process_env_step`` + ``add_transitions`` for the slot ``act`` has just written (``self.step``, then advanced): rewards[t] = rew +
        gamma * (values[t] * time_outs), dones[t] = reset, read from the task's own buffers (rew float32, reset and time_outs int64) before its next
        step rewrites them; ``obs``, the observations ``act`` was given, are copied into observations[t]."""
        need_gpu("RolloutStorage.add", rew, self.rewards)
        t = self.step
        if t >= self.T:
            raise RuntimeError("rollout storage overflow: clear() after compute_returns")
        tensor_arg(rew, torch.float32, self.n, "rew"); tensor_arg(reset, torch.long, self.n, "reset"); tensor_arg(time_outs, torch.long, self.n, "time_outs")
        if obs is not None:
            self.observations[t].copy_(obs)
        check(lib().mpc_rollout_add(self.n, float(gamma), rew.data_ptr(), reset.data_ptr(), time_outs.data_ptr(), self.values[t].data_ptr(),
                                    self.rewards[t].data_ptr(), self.dones[t].data_ptr(), _lib.stream(self.device)), "mpc_rollout_add")
        self.step += 1

    def compute_returns(self, last_values, gamma, lam):
        """``RolloutStorage.compute_returns``: GAE over the T slots into ``returns``, then ``advantages`` = returns - values normalised over all
        T N values."""
        need_gpu("RolloutStorage.compute_returns", last_values, self.rewards)
        tensor_arg(last_values, torch.float32, self.n, "last_values")
        check(lib().mpc_rollout_returns(self.n, self.T, float(gamma), float(lam), self.rewards.data_ptr(), self.dones.data_ptr(), self.values.data_ptr(),
                                        last_values.data_ptr(), self.returns.data_ptr(), self.advantages.data_ptr(), _lib.stream(self.device)),
              "mpc_rollout_returns")

    def mini_batch_generator(self, num_mini_batches, num_epochs=8):
        """rsl_rl's: one ``torch.randperm`` over T N for all epochs, mini-batch size T N // num_mini_batches.  Yields (obs, actions, values,
        advantages, returns, old log-prob, old mu, old sigma) and, with ``privileged_observations``, the critic's rows as a ninth element."""
        batch = self.n * self.T
        size = batch // num_mini_batches
        idx = torch.randperm(num_mini_batches * size, device=self.device)
        flat = [x.flatten(0, 1) for x in (self.observations, self.actions, self.values, self.advantages, self.returns, self.actions_log_prob, self.mu,
                                          self.sigma)]
        if self.privileged_observations is not None:
            flat.append(self.privileged_observations.flatten(0, 1))
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                b = idx[i * size:(i + 1) * size]
                yield tuple(x[b] for x in flat)

    def recurrent_mini_batch_generator(self, num_mini_batches, num_epochs=8):
        """rsl_rl's: mini-batches are contiguous blocks of N // num_mini_batches environments, taken in order, the same in every epoch, each with
        all the trajectories of its environments.  Yields ``RecurrentBatch``: the padded observations [T][n_traj][num_obs] (and the padded critic rows, or
        None), the masks [T][n_traj], the [T][block] slices of actions, values, advantages, returns, old log-prob, old mu and old sigma, and for each
        memory (h0, c0) [1][n_traj][H]: the saved state at each trajectory's first step (t = 0, or the step after a done)."""
        from .recurrent import RecurrentBatch, pad_trajectories, trajectory_masks
        if self.hidden is None:
            raise ValueError("the storage keeps no hidden states (RolloutStorage(hidden=))")
        block = self.n // num_mini_batches
        if block < 1:
            raise ValueError("fewer environments than mini-batches")
        masks, starts = trajectory_masks(self.dones)                               # [T][n_traj]; [N][T]: where a trajectory begins
        padded_obs = pad_trajectories(self.observations, masks)
        padded_critic = None if self.privileged_observations is None else pad_trajectories(self.privileged_observations, masks)
        first = [0] + torch.cumsum(starts.sum(dim=1), 0).tolist()                  # trajectories before environment e (one host read)
        h0 = [x.transpose(1, 0)[starts] for x in (self.saved_h_a, self.saved_c_a, self.saved_h_c, self.saved_c_c)]      # [n_traj][H], environment-major
        slices = (self.actions, self.values, self.advantages, self.returns, self.actions_log_prob, self.mu, self.sigma)
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                e0, e1 = i * block, (i + 1) * block
                k0, k1 = first[e0], first[e1]
                hid = [x[k0:k1].unsqueeze(0).contiguous() for x in h0]
                yield RecurrentBatch(padded_obs[:, k0:k1], None if padded_critic is None else padded_critic[:, k0:k1], masks[:, k0:k1],
                                     *(x[:, e0:e1] for x in slices), (hid[0], hid[1]), (hid[2], hid[3]))

    def recurrent_sequence_generator(self, num_mini_batches, num_epochs=8):
        """The dense form of ``recurrent_mini_batch_generator``: the same blocks of N // num_mini_batches environments in the same order, without
        padding, ``nonzero`` or a host read.  Yields ``RecurrentSequenceBatch``: the block's observations (and critic rows, or None) as strided views
        ``[:, e0:e1]`` of the storage, ``reset`` [T][block] int64 (reset[0] = 0, reset[t] = dones[t-1]; built once per call for all blocks), the
        [T][block] slices, and for each memory (h0, c0) = ``saved_*[0][e0:e1]``.  Equal to the padded trajectories where the saved states are zero
        after each done, which is how the collection stores them."""
        from .recurrent import RecurrentSequenceBatch
        if self.hidden is None:
            raise ValueError("the storage keeps no hidden states (RolloutStorage(hidden=))")
        block = self.n // num_mini_batches
        if block < 1:
            raise ValueError("fewer environments than mini-batches")
        reset = torch.zeros((self.T, self.n), dtype=torch.long, device=self.device)
        reset[1:] = self.dones[:-1, :, 0] != 0
        used = num_mini_batches * block
        reset = reset[:, :used].reshape(self.T, num_mini_batches, block).permute(1, 0, 2).contiguous()      # [mini-batch][T][block], dense per block
        slices = (self.actions, self.values, self.advantages, self.returns, self.actions_log_prob, self.mu, self.sigma)
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                e0, e1 = i * block, (i + 1) * block
                yield RecurrentSequenceBatch(self.observations[:, e0:e1], None if self.privileged_observations is None else self.privileged_observations[:, e0:e1],
                                             reset[i], *(x[:, e0:e1] for x in slices), (self.saved_h_a[0, e0:e1], self.saved_c_a[0, e0:e1]),
                                             (self.saved_h_c[0, e0:e1], self.saved_c_c[0, e0:e1]))

    def clear(self):
        self.step = 0


class PPO:
    """rsl_rl's ``PPO.update``.  ``backend="torch"`` (the default): plain torch (autograd + Adam) on whatever device the storage lives on.
    ``backend="hip"``: the device update of include/mpc_ppo_update.h on the same parameters, ``.grad`` tensors and optimiser state, with no host
    read: the learning rate of the adaptive schedule lives on the device (``lr_device``, float64) and ``learning_rate`` / the param groups' ``lr``
    are what the caller last copied from it (``sync_learning_rate``; ``PPOTrainer.learn`` does it once per iteration).

    A recurrent actor-critic made with ``update_heads="hip"`` takes the device path under ``backend="torch"`` (``_update_recurrent_hip``): the same
    handle over the MLPs, the memories' roll and backward pass around it, the memories' eight tensors behind the MLPs' in the clip and Adam.
    ``device_update`` says whether the update runs on the device, whichever way it was asked for; the learning rate then lives there as above."""

    def __init__(self, actor_critic, cfg=None, backend="torch"):
        if backend not in ("torch", "hip"):
            raise ValueError("backend is 'torch' or 'hip'")
        self.recurrent = bool(getattr(actor_critic, "is_recurrent", False))
        if self.recurrent and backend == "hip":                                   # (before anything asks for the device)
            raise ValueError('PPO(backend="hip") with a recurrent actor-critic: the MLPs, the loss head and Adam of a recurrent device update are not built (the '
                             'memories\' update through time is: RecurrentConfig(update_through_time="hip")); use backend="torch"')
        self.cfg = cfg if cfg is not None else PPOConfig()
        self.actor_critic = actor_critic
        self.backend = backend
        self.device_update = backend == "hip" or (self.recurrent and getattr(actor_critic, "update_heads", "torch") == "hip")
        self.learning_rate = float(self.cfg.learning_rate)
        self.optimizer = torch.optim.Adam(actor_critic.parameters(), lr=self.learning_rate)
        self.last_terms = None
        self._handle, self._max_rows, self._bound, self._storage_ptrs, self._ac_ptrs = None, 0, None, None, None
        self.lr_device, self.record_lr, self.lr_trace = None, False, None       # record_lr (for tests): keep the rate after every decision in lr_trace
        self._extra_bound, self._seq_rows, self._seq_ptrs, self._seq_store = None, None, None, None      # (the recurrent device update's: the memories' binding, the dense buffers)
        if self.device_update:
            need_gpu('PPO(backend="hip")' if backend == "hip" else 'PPO on update_heads="hip"', actor_critic.std)
            group = self.optimizer.param_groups[0]
            if group["amsgrad"] or group["weight_decay"] != 0 or group["maximize"]:
                raise ValueError("the device update restates plain Adam: no amsgrad, weight decay or maximize")
            update_lib()
            self.lr_device = torch.full((1,), self.learning_rate, dtype=torch.float64, device=actor_critic.std.device)

    __del__ = _lib.finalizer("mpc_ppo_update_destroy")

    def adapt_learning_rate(self, kl_mean):
        """The adaptive schedule: lr / 1.5 (not below 1e-5) if kl > 2 desired_kl, lr * 1.5 (not above 1e-2) if 0 < kl < desired_kl / 2."""
        c = self.cfg
        if kl_mean > c.desired_kl * 2.0:
            self.learning_rate = max(1e-5, self.learning_rate / 1.5)
        elif kl_mean < c.desired_kl / 2.0 and kl_mean > 0.0:
            self.learning_rate = min(1e-2, self.learning_rate * 1.5)
        for group in self.optimizer.param_groups:
            group["lr"] = self.learning_rate

    def losses(self, batch):
        """(surrogate, value loss, mean entropy, mean kl) of one mini-batch of ``RolloutStorage.mini_batch_generator``; kl carries no gradient.  On a
        recurrent actor-critic: of one ``RecurrentBatch`` of ``recurrent_mini_batch_generator``, the same formulas, the means over all T x block elements."""
        c = self.cfg
        if self.recurrent:
            b = batch
            form = {"reset": b.reset} if hasattr(b, "reset") else {"masks": b.masks}      # the dense roll (recurrent_sequence_generator) or padded trajectories
            out = self.actor_critic.log_prob_entropy_value(b.obs, b.actions, b.critic_obs, hidden_states=(b.hidden_a, b.hidden_c), **form)
            logp, entropy, value, mu, sigma = (x.flatten(0, 1) for x in out)       # [T][block][..] -> [T block][..], as the feed-forward batch has them
            actions, old_values, adv, returns, old_logp, old_mu, old_sigma = (x.flatten(0, 1) for x in (b.actions, b.values, b.advantages, b.returns,
                                                                                                        b.old_log_prob, b.old_mu, b.old_sigma))
        else:
            obs, actions, old_values, adv, returns, old_logp, old_mu, old_sigma = batch[:8]
            critic_obs = batch[8] if len(batch) > 8 else None                    # the critic's rows, when the storage keeps them
            if critic_obs is None and self.actor_critic.num_critic_obs is not None:
                raise ValueError("the actor-critic was made with num_critic_obs and the batch carries no critic rows (RolloutStorage(num_privileged_obs=))")
            logp, entropy, value, mu, sigma = self.actor_critic.log_prob_entropy_value(obs, actions, critic_obs)
        with torch.no_grad():
            kl = torch.sum(torch.log(sigma / old_sigma + 1.e-5) + (torch.square(old_sigma) + torch.square(old_mu - mu)) / (2.0 * torch.square(sigma)) - 0.5,
                           axis=-1).mean()
        ratio = torch.exp(logp - torch.squeeze(old_logp))
        a = torch.squeeze(adv)
        surrogate = torch.max(-a * ratio, -a * torch.clamp(ratio, 1.0 - c.clip_param, 1.0 + c.clip_param)).mean()
        if c.use_clipped_value_loss:
            clipped = old_values + (value - old_values).clamp(-c.clip_param, c.clip_param)
            value_loss = torch.max((value - returns).pow(2), (clipped - returns).pow(2)).mean()
        else:
            value_loss = (returns - value).pow(2).mean()
        return surrogate, value_loss, entropy.mean(), kl

    # ---- the device update ----------------------------------------------------------------------------------------------------------
    def set_learning_rate(self, lr):
        """Sets the learning rate everywhere it lives: here, in the param groups and (hip backend) on the device."""
        self.learning_rate = float(lr)
        for group in self.optimizer.param_groups:
            group["lr"] = self.learning_rate
        if self.lr_device is not None:
            self.lr_device.fill_(self.learning_rate)

    def sync_learning_rate(self, lr=None):
        """hip backend: ``learning_rate`` and the param groups' ``lr`` from the device value (``lr``: that value if the caller has fetched it
        already, otherwise it is read here, which waits for the device)."""
        self.learning_rate = float(self.lr_device.item() if lr is None else lr)
        for group in self.optimizer.param_groups:
            group["lr"] = self.learning_rate

    def workspace_bytes(self):
        """Device memory behind the device update as it stands: the handle's workspace and, on a recurrent actor-critic, the four dense row buffers
        (the memories' own workspace is ``actor_critic._seq.workspace_bytes()``).  0 before the first update."""
        own = 0 if self._handle is None else int(update_lib().mpc_ppo_update_workspace_bytes(self._handle))
        return own + (0 if self._seq_store is None else sum(4 * t.numel() for t in self._seq_store))

    def _device_state(self, rows, extra=()):
        """The handle, sized for ``rows`` and bound to the current addresses of the gradients and moments (created here, on the first step, as
        torch creates them); returns the common step count.  ``extra``: the parameters that go behind the ``mpc_ac``'s (``mpc_ppo_update_bind_extra``)."""
        ac = self.actor_critic
        dev = ac.std.device
        ac._ready("PPO.update", torch.empty((1, ac.num_obs), dtype=torch.float32, device=dev))      # (the handle and its binding: nothing is launched)
        params = ac.bind_order()
        extra = list(extra)
        steps = set()
        for p in params + extra:
            st = self.optimizer.state[p]
            if len(st) == 0:                                                      # torch.optim.Adam._init_group
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif st["step"].is_cuda:                                             # (a checkpoint loaded with map_location: one read, then it is the host's)
                st["step"] = st["step"].cpu()
            steps.add(int(st["step"]))
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        if len(steps) != 1:
            raise ValueError("the device update steps every parameter together: the optimiser's step counts differ")
        if self._handle is None or rows > self._max_rows or self._ac_ptrs != ac._bound_ptrs:
            if self._handle is not None:
                update_lib().mpc_ppo_update_destroy(self._handle)
                self._handle = None
            h = C.c_void_p()
            with torch.cuda.device(dev):
                check(update_lib().mpc_ppo_update_create(C.byref(h), ac._handle, int(rows)), "mpc_ppo_update_create")
            self._handle, self._max_rows, self._bound, self._storage_ptrs, self._ac_ptrs = h, int(rows), None, None, ac._bound_ptrs
            self._extra_bound, self._seq_ptrs = None, None
        tensors = [p.grad for p in params] + [self.optimizer.state[p][key] for key in ("exp_avg", "exp_avg_sq") for p in params]
        ptrs = _lib.addresses_to_bind(tensors, self._bound, dev, "gradients and Adam's moments must be contiguous float32 tensors shaped like their parameters, on their device",
                                      like=3 * params)
        if ptrs is not None:
            n, arr = len(params), _lib.ptr_array
            check(update_lib().mpc_ppo_update_bind(self._handle, arr(ptrs[:n]), arr(ptrs[n:2 * n]), arr(ptrs[2 * n:])), "mpc_ppo_update_bind")
            self._bound = ptrs
        if extra:
            tensors = extra + [p.grad for p in extra] + [self.optimizer.state[p][key] for key in ("exp_avg", "exp_avg_sq") for p in extra]
            ptrs = _lib.addresses_to_bind(tensors, self._extra_bound, dev, "the memories' parameters, gradients and Adam's moments must be contiguous float32 tensors "
                                          "shaped like their parameters, on the MLPs' device", like=4 * extra)
            if ptrs is not None:
                n, arr = len(extra), _lib.ptr_array
                with torch.cuda.device(dev):
                    check(update_lib().mpc_ppo_update_bind_extra(self._handle, n, arr(ptrs[:n]), arr(ptrs[n:2 * n]), arr(ptrs[2 * n:3 * n]), arr(ptrs[3 * n:]),
                                                                 _lib.int_array([p.numel() for p in extra])), "mpc_ppo_update_bind_extra")
                self._extra_bound = ptrs
        return steps.pop()

    def _update_hip(self, storage, indices=None):
        c = self.cfg
        dev = self.actor_critic.std.device
        need_gpu("PPO.update", storage.observations, self.actor_critic.std)
        if storage.device != dev:
            raise _lib.MpcLibraryError("PPO.update: the storage and the parameters live on different devices")
        total = storage.n * storage.T
        size = total // c.num_mini_batches
        if size < 1:
            raise ValueError("fewer rows than mini-batches")
        if indices is None:
            indices = torch.randperm(c.num_mini_batches * size, device=dev)
        tensor_arg(indices, torch.long, c.num_mini_batches * size, "indices")
        step = self._device_state(size)
        L = update_lib()
        flat = (storage.observations, storage.actions, storage.values, storage.advantages, storage.returns, storage.actions_log_prob, storage.mu, storage.sigma)
        widths = (self.actor_critic.num_obs, NUM_ACTIONS, 1, 1, 1, 1, NUM_ACTIONS, NUM_ACTIONS)
        ptrs = tuple(tensor_arg(t, torch.float32, total * w, "storage").data_ptr() for t, w in zip(flat, widths))
        critic_rows = storage.privileged_observations                            # None on a symmetric run: today's calls and no other
        if critic_rows is not None:
            ptrs += (tensor_arg(critic_rows, torch.float32, total * self.actor_critic.critic_width, "storage.privileged_observations").data_ptr(),)
        if ptrs != self._storage_ptrs:
            check(L.mpc_ppo_update_set_storage(self._handle, total, *ptrs[:8]), "mpc_ppo_update_set_storage")
            if critic_rows is not None or (self._storage_ptrs is not None and len(self._storage_ptrs) > 8):      # set, or cleared after a storage that had them
                check(L.mpc_ppo_update_set_critic_storage(self._handle, ptrs[8] if critic_rows is not None else None), "mpc_ppo_update_set_critic_storage")
            self._storage_ptrs = ptrs
        adaptive = c.desired_kl is not None and c.schedule == "adaptive"
        group = self.optimizer.param_groups[0]
        beta1, beta2 = group["betas"]
        k = c.num_learning_epochs * c.num_mini_batches
        terms = torch.empty((k, 4), dtype=torch.float32, device=dev)
        if self.record_lr:
            self.lr_trace = torch.empty(k, dtype=torch.float64, device=dev)
        stream = _lib.stream(dev)
        params = self.actor_critic.bind_order()
        with torch.cuda.device(dev):
            for e in range(c.num_learning_epochs):
                for i in range(c.num_mini_batches):
                    j = e * c.num_mini_batches + i
                    check(L.mpc_ppo_update_grads(self._handle, size, indices.data_ptr() + 8 * i * size, float(c.clip_param), float(c.value_loss_coef),
                                                 float(c.entropy_coef), int(bool(c.use_clipped_value_loss)), int(adaptive),
                                                 float(c.desired_kl) if adaptive else 0.0, self.lr_device.data_ptr(), terms[j].data_ptr(), stream),
                          "mpc_ppo_update_grads")
                    if self.record_lr:
                        self.lr_trace[j:j + 1].copy_(self.lr_device)
                    step += 1
                    check(L.mpc_ppo_update_apply(self._handle, float(c.max_grad_norm), float(beta1), float(beta2), float(group["eps"]), step,
                                                 self.lr_device.data_ptr(), stream), "mpc_ppo_update_apply")
        for p in params:
            self.optimizer.state[p]["step"] += float(k)                          # (host tensors: no device work)
        self.last_terms = tuple(terms[k - 1, q] for q in range(4))
        storage.clear()
        return terms[:, 1].mean(), terms[:, 0].mean()

    def _recurrent_plan(self, storage):
        """What one update of ``_update_recurrent_hip`` sets up, once, on the device and with no host read: the handle bound to all tensors (the
        memories' eight behind the MLPs'), the storage and the four persistent ``[T B][H]`` buffers ``_seq_rows`` = (y_a, y_c, dy_a, dy_c) set on it,
        the reset flags ``[mini-batch][T][B]`` as ``recurrent_sequence_generator`` builds them and the row index ``idx[i][t B + b] = t N + i B + b``.
        Returns a dict for ``_recurrent_grads``; ``step`` is the optimiser's common step count."""
        from .recurrent import SequenceKernel
        c, ac = self.cfg, self.actor_critic
        dev = ac.std.device
        need_gpu("PPO.update", storage.observations, ac.std)
        if storage.device != dev:
            raise _lib.MpcLibraryError("PPO.update: the storage and the parameters live on different devices")
        if storage.hidden is None:
            raise ValueError("the storage keeps no hidden states (RolloutStorage(hidden=))")
        T, N, mb, H = storage.T, storage.n, c.num_mini_batches, ac.rnn_hidden_size
        B = N // mb
        if B < 1:
            raise ValueError("fewer environments than mini-batches")
        rows, total = T * B, T * N
        critic_rows = storage.privileged_observations
        if critic_rows is None:
            if ac.privileged:
                raise ValueError("the actor-critic was made with num_critic_obs and the storage keeps no critic rows (RolloutStorage(num_privileged_obs=))")
            critic_rows = storage.observations
        memory_params = [p for m in ac.memories() for p in m.parameters_in_bind_order()]
        step = self._device_state(rows, extra=memory_params)
        L = update_lib()
        flat = (storage.observations, storage.actions, storage.values, storage.advantages, storage.returns, storage.actions_log_prob, storage.mu, storage.sigma)
        widths = (ac.obs_width, NUM_ACTIONS, 1, 1, 1, 1, NUM_ACTIONS, NUM_ACTIONS)
        ptrs = tuple(tensor_arg(t, torch.float32, total * w, "storage").data_ptr() for t, w in zip(flat, widths))
        if ptrs != self._storage_ptrs:                                            # (d_obs names the storage; the sequence call does not read it)
            check(L.mpc_ppo_update_set_storage(self._handle, total, *ptrs), "mpc_ppo_update_set_storage")
            self._storage_ptrs = ptrs
        grown = self._seq_store is not None and self._seq_store[0].shape[0] < self._max_rows      # (a new handle for more rows)
        if self._seq_rows is None or grown or any(t.shape != (rows, H) or t.device != dev for t in self._seq_rows):
            cap = self._max_rows                                                 # the handle's: what set_sequence_rows takes every buffer to hold
            if self._seq_store is None or any(t.shape[0] < cap or t.shape[1] != H or t.device != dev for t in self._seq_store):
                self._seq_store = tuple(torch.zeros((cap, H), dtype=torch.float32, device=dev) for _ in range(4))
            self._seq_rows = tuple(t[:rows] for t in self._seq_store)
        seq_ptrs = tuple(tensor_arg(t, torch.float32, rows * H, "a dense row buffer").data_ptr() for t in self._seq_rows)
        if seq_ptrs != self._seq_ptrs:
            check(L.mpc_ppo_update_set_sequence_rows(self._handle, *seq_ptrs), "mpc_ppo_update_set_sequence_rows")
            self._seq_ptrs = seq_ptrs
        if ac._seq is None:
            ac._seq = SequenceKernel(ac.memories())
        used = mb * B
        reset = torch.zeros((T, N), dtype=torch.long, device=dev)
        reset[1:] = storage.dones[:-1, :, 0] != 0
        reset = reset[:, :used].reshape(T, mb, B).permute(1, 0, 2).contiguous()
        t_, b_, i_ = (torch.arange(n, dtype=torch.long, device=dev) for n in (T, B, mb))
        idx = ((t_[:, None] * N + b_[None, :]).reshape(1, rows) + (i_ * B)[:, None]).contiguous()
        return dict(T=T, B=B, rows=rows, mini_batches=mb, step=step, reset=reset, idx=idx, obs=storage.observations, critic_rows=critic_rows,
                    h0=(storage.saved_h_a, storage.saved_h_c), c0=(storage.saved_c_a, storage.saved_c_c), memory_params=memory_params,
                    memory_grads=[[p.grad for p in m.parameters_in_bind_order()] for m in ac.memories()], stream=_lib.stream(dev),
                    adaptive=c.desired_kl is not None and c.schedule == "adaptive")

    def _recurrent_grads(self, plan, i, terms):
        """Mini-batch ``i`` of ``plan`` up to the gradients: the forward roll into (y_a, y_c), ``mpc_ppo_update_grads_sequence`` (the MLPs' and std's
        ``.grad``, ``terms`` [4], the learning-rate decision, (dy_a, dy_c)), the backward pass through time into the memories' ``.grad``."""
        from .recurrent import ACTOR, CRITIC
        c, seq, which = self.cfg, self.actor_critic._seq, (ACTOR, CRITIC)
        y_a, y_c, dy_a, dy_c = self._seq_rows
        T, B = plan["T"], plan["B"]
        e0, e1 = i * B, (i + 1) * B
        token = seq.token + 1                                                    # the forward call below: what the backward call must go back through
        seq.forward(which, (plan["obs"][:, e0:e1], plan["critic_rows"][:, e0:e1]), [h[0, e0:e1] for h in plan["h0"]], [x[0, e0:e1] for x in plan["c0"]],
                    plan["reset"][i], what='update_heads="hip"', out=((y_a, None), (y_c, None)))
        adaptive = plan["adaptive"]
        check(update_lib().mpc_ppo_update_grads_sequence(self._handle, plan["rows"], plan["idx"][i].data_ptr(), float(c.clip_param), float(c.value_loss_coef),
                                                         float(c.entropy_coef), int(bool(c.use_clipped_value_loss)), int(adaptive),
                                                         float(c.desired_kl) if adaptive else 0.0, self.lr_device.data_ptr(), terms.data_ptr(), plan["stream"]),
              "mpc_ppo_update_grads_sequence")
        seq.backward(which, T, B, (dy_a, dy_c), token, out=plan["memory_grads"])      # (overwrites the memories' .grad)

    def _update_recurrent_hip(self, storage):
        """``update_heads="hip"``: per mini-batch ``_recurrent_grads`` and one ``mpc_ppo_update_apply`` over the MLPs' and the memories' tensors -- on one
        stream, with no host read and no autograd.  The mini-batches are ``recurrent_sequence_generator``'s: blocks of N // num_mini_batches
        environments in order, the same in every epoch, the left-over dropped."""
        c, ac = self.cfg, self.actor_critic
        dev = ac.std.device
        plan = self._recurrent_plan(storage)
        mb, step = plan["mini_batches"], plan["step"]
        group = self.optimizer.param_groups[0]
        beta1, beta2 = group["betas"]
        k = c.num_learning_epochs * mb
        terms = torch.empty((k, 4), dtype=torch.float32, device=dev)
        if self.record_lr:
            self.lr_trace = torch.empty(k, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            for e in range(c.num_learning_epochs):
                for i in range(mb):
                    j = e * mb + i
                    self._recurrent_grads(plan, i, terms[j])
                    if self.record_lr:
                        self.lr_trace[j:j + 1].copy_(self.lr_device)
                    step += 1
                    check(update_lib().mpc_ppo_update_apply(self._handle, float(c.max_grad_norm), float(beta1), float(beta2), float(group["eps"]), step,
                                                            self.lr_device.data_ptr(), plan["stream"]), "mpc_ppo_update_apply")
        for p in ac.bind_order() + plan["memory_params"]:
            self.optimizer.state[p]["step"] += float(k)                          # (host tensors: no device work)
        self.last_terms = tuple(terms[k - 1, q] for q in range(4))
        storage.clear()
        return terms[:, 1].mean(), terms[:, 0].mean()

    def update(self, storage, indices=None):
        """One update over the storage: num_learning_epochs x num_mini_batches Adam steps.  Returns device tensors (mean value loss, mean
        surrogate loss).  torch backend: the only host read per mini-batch is the kl of the adaptive schedule (as in rsl_rl).  hip backend: no host
        read at all; ``indices`` (for tests) replaces the ``torch.randperm`` over the num_mini_batches * (T N // num_mini_batches) rows."""
        if self.backend == "hip":
            return self._update_hip(storage, indices)
        if self.device_update:                                                   # a recurrent actor-critic with update_heads="hip"
            if indices is not None:
                raise ValueError("indices are taken by the hip backend only")
            return self._update_recurrent_hip(storage)
        if indices is not None:
            raise ValueError("indices are taken by the hip backend only")
        c = self.cfg
        mean_value, mean_surrogate, k = 0.0, 0.0, 0
        generator = storage.recurrent_mini_batch_generator if self.recurrent else storage.mini_batch_generator
        if self.recurrent and getattr(self.actor_critic, "update_through_time", "torch") == "hip":
            generator = storage.recurrent_sequence_generator                      # the memories' update through time on the device: the dense roll
        for batch in generator(c.num_mini_batches, c.num_learning_epochs):
            surrogate, value_loss, entropy, kl = self.losses(batch)
            if c.desired_kl is not None and c.schedule == "adaptive":
                self.adapt_learning_rate(kl.item())
            loss = surrogate + c.value_loss_coef * value_loss - c.entropy_coef * entropy
            self.optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(self.actor_critic.parameters(), c.max_grad_norm)
            self.optimizer.step()
            self.last_terms = (surrogate.detach(), value_loss.detach(), entropy.detach(), kl)
            mean_value, mean_surrogate, k = mean_value + value_loss.detach(), mean_surrogate + surrogate.detach(), k + 1
        storage.clear()
        return mean_value / k, mean_surrogate / k


class _Rows:
    """One stream of rows from the environment to the nets.  ``source(returned)``: the raw rows after ``returned = env.reset()`` or ``env.step()[0]`` (the
    actor's are ``returned``, the critic's ``env.privileged_obs_buf``); ``storage`` [T, N, W]: the rollout's tensor for them; ``norm``: an ``ObsNormalizer``
    or None; ``held`` [N, W]: the normalised rows between collections."""

    def __init__(self, source, storage, norm=None):
        self.source, self.storage, self.norm = source, storage, norm
        self.held = None if norm is None else torch.zeros_like(storage[0])

    def read(self, returned, t=None, update=True):
        """The rows the environment has just produced: as they are, or counted (``update=False``, an evaluation: the statistics stay) and normalised once,
        by a launch that writes where a ``copy_`` would have -- after the step of slot ``t`` into ``storage[t + 1]``, which the next tick reads; after
        the last slot, after ``reset()`` and in an evaluation (``t`` None) into ``held``."""
        rows = self.source(returned)
        if self.norm is None:
            return rows
        return self.norm(rows, out=self.storage[t + 1] if t is not None and t + 1 < len(self.storage) else self.held, update=update)

    def keep(self, t, rows):
        """The rows slot t's action and value were computed from, into ``storage[t]`` -- unless ``read`` normalised them into it."""
        if self.norm is None or t == 0:
            self.storage[t].copy_(rows)


# What rides along in the one host read of an iteration: ``summary()`` -> a 1-D float64 device tensor (or None: nothing to read), ``record(values)``
# -> the entries its slice of the read adds to the iteration's record, ``after()`` -> what follows the read.  Called through the objects at use time.
_Rider = namedtuple("_Rider", "summary record after", defaults=(None,))
SCALARS = ("mean_reward", "done_rate", "value_loss", "surrogate_loss", "mean_noise_std")


def episode_record(s):
    """``EpisodeStats.summary``'s values as a record's entries: rsl_rl's statistics over the last 100 finished episodes."""
    return dict(mean_episode_return=s[S_MEAN_RETURN], mean_episode_length=s[S_MEAN_LENGTH], episodes_in_window=int(s[S_WINDOW_COUNT]),
                episodes_finished=int(s[S_EPISODES]), timeouts_in_window=int(s[S_WINDOW_TIMEOUTS]))


def _riders(trainer):
    """The riders of ``trainer`` (anything with its ``_scalars``, ``alg``, ``episode_stats``, ``curriculum`` and ``episode_terms``; ``reward_shaping`` and
    ``contact_terms`` where it has one), in the record's order."""
    alg, curriculum, terms, shaping = trainer.alg, trainer.curriculum, trainer.episode_terms, getattr(trainer, "reward_shaping", None)
    contact = getattr(trainer, "contact_terms", None)

    def learning_rate(values):                                                   # a device update: the device's value, which the host copies follow
        if values:
            alg.sync_learning_rate(values[0])
        return {"learning_rate": alg.learning_rate}

    riders = [_Rider(lambda: trainer._scalars, lambda values: dict(zip(SCALARS, values))),
              _Rider(lambda: alg.lr_device, learning_rate),                    # (None on the torch backend)
              _Rider(lambda: trainer.episode_stats.summary, episode_record)]
    if curriculum is not None:                                                   # the terrain levels as they stand after the iteration
        riders.append(_Rider(lambda: curriculum.summary(), lambda values: curriculum.record(values, curriculum.num_types)))
    if terms is not None:                                                        # the per-term sums of the iteration's closed episodes; the next record covers the next
        riders.append(_Rider(lambda: terms.summary(), lambda values: {"episode_terms": terms.record(values)}, lambda: terms.new_window()))
    if shaping is not None:                                                      # the shaping terms' sums of the iteration's closed episodes, window by window
        riders.append(_Rider(lambda: shaping.summary(), lambda values: {"reward_shaping": shaping.record(values)}, lambda: shaping.new_window()))
    if contact is not None:                                                      # the contact terms' sums, in the same way
        riders.append(_Rider(lambda: contact.summary(), lambda values: {"contact_terms": contact.record(values)}, lambda: contact.new_window()))
    return riders


def _read_riders(riders):
    """The riders' summaries in ONE host read, each rider's own values to its ``record``: the entries of the iteration's record, in the riders' order."""
    parts = [r.summary() for r in riders]
    flat = iter(torch.cat([p for p in parts if p is not None]).tolist())
    record = {}
    for r, p in zip(riders, parts):
        record.update(r.record(list(islice(flat, 0 if p is None else p.numel()))))
        if r.after is not None:
            r.after()
    return record


# A part of the checkpoint beside the model and the optimiser: ``obj`` (None: this trainer has none) is saved under ``key`` and loaded when both sides
# have it, ``after()`` follows a load.  ``missing`` / ``unexpected``: the error when only the trainer / only the checkpoint has it (None: no error).
_Part = namedtuple("_Part", "key obj missing unexpected after", defaults=(None, None, None))


def _checkpoint_parts(trainer):
    """The parts of ``trainer`` (anything with its ``obs_norm``, ``critic_obs_norm``, ``episode_terms``, ``plant_rand``, ``env`` and ``obs``; ``friction`` where
    it has one), in the checkpoint's order."""
    env, terms = trainer.env, trainer.episode_terms

    def forget_obs():                                                            # (normalised with the statistics before the load)
        trainer.obs = None

    def set_clock():                                                             # the command curriculum's clock follows the checkpoint's
        if hasattr(env, "common_step_counter"):
            env.common_step_counter = terms.tick
    # (the friction first: both of its refusals come before any part has been loaded)
    return (_Part("friction_state_dict", getattr(trainer, "friction", None), "this trainer's environment has friction and the checkpoint carries no friction_state_dict",
                  "the checkpoint was written with friction (friction_state_dict) and this trainer's environment has none"),
            _Part("obs_norm_state_dict", trainer.obs_norm, "this trainer normalises observations and the checkpoint carries no obs_norm_state_dict",
                  "the checkpoint was written with observation normalisation and this trainer has none", forget_obs),
            _Part("critic_obs_norm_state_dict", trainer.critic_obs_norm,
                  "this trainer normalises the critic's rows and the checkpoint carries no critic_obs_norm_state_dict"),
            _Part("episode_terms_state_dict", terms, after=set_clock),         # the command range the policy was trained up to
            _Part("plant_rand_state_dict", trainer.plant_rand))                # the plants the rollouts continue on


def _save_parts(parts, ck):
    ck.update({p.key: p.obj.state_dict() for p in parts if p.obj is not None})


def _load_parts(parts, ck):
    for p in parts:
        have, held = p.obj is not None, p.key in ck
        error = p.missing if have else p.unexpected
        if have != held and error is not None:
            raise ValueError(error)
        if have and held:
            p.obj.load_state_dict(ck[p.key])
            if p.after is not None:
                p.after()


class PPOTrainer:
    """rsl_rl's ``OnPolicyRunner`` for an environment with ``BatchedRLTask``'s members: ``num_envs``, ``num_obs``, ``num_actions``, ``reset()``,
    ``step(actions) -> (obs, rew, reset, extras)`` with ``extras["time_outs"]`` (rew float32, reset and time_outs int64, cuda).

    An iteration: T times ``act`` into slot t, ``env.step``, ``add``; then ``evaluate`` and ``compute_returns`` -- nothing of that is copied to
    the host or waits for the device -- and ``PPO.update``.  ``seed`` seeds torch's global generator (weight initialisation, the update's
    ``randperm``), as the reference's train.py does, and the exploration noise.  Every option is opt-in, found on the environment with ``getattr`` or
    asked for here; without it the launches are the plain trainer's.  Each states once what it adds to one of four things:

    **Rows** (``_Rows``).  The actor's are what the environment returns (``self.obs``).  An environment with ``num_privileged_obs``
    (``BatchedRLTask(privileged_obs=...)``) trains an asymmetric actor-critic: the critic's first layer is that wide and reads each tick's
    ``env.privileged_obs_buf`` (``self.critic_obs``; None otherwise), kept in ``storage.privileged_observations[t]``; ``last_values`` is the critic's of
    the last such row.  ``normalize_obs=True`` puts an ``ObsNormalizer`` into each stream (``obs_norm``, ``critic_obs_norm``; ``obs_norm_eps``,
    ``obs_norm_until`` are their ``eps`` and ``until``): every row is counted once and normalised once with the statistics that include it, and ``act``,
    the storage, ``evaluate`` and both update backends see the normalised tensor; ``evaluate`` and ``get_inference_policy`` normalise without updating.
    A constant column of the critic's rows (the zero pad, a contact flag that never changes) has zero variance and normalises to 0 / eps = 0.

    **Riders** (``_riders``) of an iteration's one host read, each with the entries it adds to the record (``learn``).  **Checkpoint parts**
    (``_checkpoint_parts``) beside the model and the optimiser (``save``).  A new option supplies a rider, a part, or a stream of rows.

    **Memory.**  ``recurrent=RecurrentConfig(hidden_size=...)`` (``recurrent.py``) trains an ``ActorCriticRecurrent``: each tick's ``act`` is handed
    the task's reset tensor of the tick before (the memories start an episode from zero state) and slot t's views of the storage's saved hidden states
    -- nothing more is copied per tick -- and the update is the torch one over padded trajectories, or, with
    ``RecurrentConfig(update_through_time="hip")``, torch's MLPs, loss and Adam around the memories' roll and backward pass on the device, or, with
    ``update_heads="hip"`` as well, all of it on the device with no host read per mini-batch (``PPO._update_recurrent_hip``).  The memories
    read what the MLPs' first layers read otherwise.  ``update="hip"`` is refused.  A feed-forward actor-critic is called the same way and handed None."""

    def __init__(self, env, cfg=None, seed=1, device=None, update="torch", normalize_obs=False, obs_norm_eps=1e-2, obs_norm_until=None, recurrent=None):
        if recurrent is not None and update == "hip":                            # (PPO's own refusal, before the device is asked for)
            raise ValueError('PPOTrainer(update="hip") with recurrent=: the MLPs, the loss head and Adam of a recurrent device update are not built (the memories\' '
                             'update through time is: RecurrentConfig(update_through_time="hip")); use update="torch"')
        need_gpu("PPOTrainer")
        self.cfg = cfg if cfg is not None else PPOConfig()
        self.env, self.seed = env, int(seed)
        self.device = _lib.device_of(device if device is not None else getattr(env, "device", None))
        torch.manual_seed(self.seed)
        c = self.cfg
        self.num_privileged_obs, self.curriculum, self.episode_terms, self.plant_rand, self.reward_shaping, self.friction, self.contact_terms = (
            getattr(env, name, None) for name in ("num_privileged_obs", "curriculum", "episode_terms", "plant_rand", "reward_shaping", "friction", "contact_terms"))
        priv = self.num_privileged_obs
        self.recurrent = recurrent
        self._prev_reset = None                                                  # the task's reset tensor of the tick before (kept for a net with memory only)
        nets = dict(num_obs=env.num_obs, num_actions=env.num_actions, actor_hidden_dims=c.actor_hidden_dims, critic_hidden_dims=c.critic_hidden_dims,
                    init_noise_std=c.init_noise_std, num_critic_obs=priv)
        if recurrent is not None:
            from .recurrent import ActorCriticRecurrent
            nets.update(rnn_type=recurrent.rnn_type, rnn_hidden_size=recurrent.hidden_size, rnn_num_layers=recurrent.num_layers,
                        update_through_time=getattr(recurrent, "update_through_time", "torch"), update_heads=getattr(recurrent, "update_heads", "torch"))
        self.actor_critic = (ActorCritic if recurrent is None else ActorCriticRecurrent)(**nets).to(self.device)
        self.alg = PPO(self.actor_critic, c, backend=update)
        self.storage = RolloutStorage(env.num_envs, c.num_steps_per_env, self.device, env.num_obs, env.num_actions, num_privileged_obs=priv,
                                      hidden=self.actor_critic.hidden_sizes)
        self.episode_stats = EpisodeStats(env.num_envs, device=self.device)      # rsl_rl's rewbuffer / lenbuffer (deque(maxlen=100)), on the device
        self.iteration, self.tick, self.obs = 0, 0, None
        self.critic_obs = None                                                   # the critic's rows that go with self.obs (None without privileged observations)
        self.infos = []
        norm = lambda width: ObsNormalizer(width, eps=obs_norm_eps, until=obs_norm_until, device=self.device) if normalize_obs else None
        self._rows = _Rows(lambda returned: returned, self.storage.observations, norm(env.num_obs))
        self._critic_rows = None if priv is None else _Rows(lambda _: env.privileged_obs_buf, self.storage.privileged_observations, norm(priv))
        self.obs_norm, self.critic_obs_norm = self._rows.norm, None if priv is None else self._critic_rows.norm
        self._scalars = None                                                     # the iteration's five scalars (float64, on the device) for the read
        self._riders = _riders(self)

    def _first_obs(self):
        """``env.reset()``'s observation, normalised (and counted) when normalisation is on; ``critic_obs`` follows it."""
        returned = self.env.reset()
        if self._critic_rows is not None:
            self.critic_obs = self._critic_rows.read(returned)
        return self._rows.read(returned)

    def collect(self, record_eps=None):
        """The collection half of one iteration (T ticks), entirely on the device.  ``record_eps``: a list that receives each tick's noise."""
        c, st, rows, critic_rows = self.cfg, self.storage, self._rows, self._critic_rows
        if self.obs is None:
            self.obs = self._first_obs()
        st.clear()
        with torch.no_grad():
            for t in range(st.T):                                                # (the memories' state of slot t goes straight into the storage)
                out = self.actor_critic.act(self.obs, self.seed, self.tick, out=st.slot(t), return_eps=record_eps is not None, critic_obs=self.critic_obs,
                                            reset=self._prev_reset, saved=st.hidden_slot(t))
                if record_eps is not None:
                    record_eps.append(out["eps"])
                rows.keep(t, self.obs)
                if critic_rows is not None:
                    critic_rows.keep(t, self.critic_obs)
                returned, rew, reset, extras = self.env.step(st.actions[t])
                if st.hidden is not None:                                        # (the task's own buffer: read by the next cell launch, before the next step rewrites it)
                    self._prev_reset = reset
                self.obs = rows.read(returned, t)
                if critic_rows is not None:                                      # the task's own buffer, rewritten by its next step; or its normalised copy
                    self.critic_obs = critic_rows.read(returned, t)
                st.add(rew, reset, extras["time_outs"], c.gamma)
                self.episode_stats.add(rew, reset, extras["time_outs"])
                self.tick += 1
            self.last_values = self.actor_critic.evaluate(self.obs if critic_rows is None else self.critic_obs, reset=self._prev_reset)
            st.compute_returns(self.last_values, c.gamma, c.lam)

    def learn(self, num_iterations, init_at_random_ep_len=False):
        """``num_iterations`` of collection + update.  Appends one record per iteration to ``infos`` (read from the device once, after the
        update) and returns the list.  Besides the losses a record carries rsl_rl's episode statistics: ``mean_episode_return`` and
        ``mean_episode_length`` over the last 100 finished episodes (0.0 while there are none), ``episodes_in_window``, ``timeouts_in_window`` and
        the cumulative ``episodes_finished``; on an environment with a terrain ``curriculum`` also ``mean_terrain_level`` and ``terrain_level_by_type``
        as they stand after the iteration; on one with ``episode_terms`` also ``episode_terms``: ``rew_<term>`` over the episodes closed during the
        iteration, ``max_command_x``, ``min_command_x`` and ``command_widenings`` (``EpisodeTerms.record``); on one with ``reward_shaping`` also ``reward_shaping``: ``rew_<term>`` of the eight shaping terms over
        the episodes closed during the iteration (``RewardShaping.record``); on one with ``contact_terms`` also ``contact_terms``: ``rew_<term>`` of the three contact terms
        (``ContactTerms.record``).  ``init_at_random_ep_len``: before the first collection ``env.progress_buf`` is set to integers
        uniform on [0, ``env.cfg.max_episode_length``), drawn from the trainer's seed, so that the environments do not time out on one tick.  As in
        rsl_rl's ``learn``, this happens at the start of EVERY call that sets the flag (the same draw each time: it moves episodes that are under way),
        so set it on the first call only."""
        if init_at_random_ep_len:
            progress, max_len = getattr(self.env, "progress_buf", None), getattr(getattr(self.env, "cfg", None), "max_episode_length", None)
            if progress is None or max_len is None:
                raise ValueError("init_at_random_ep_len needs an environment with progress_buf and cfg.max_episode_length")
            if self.obs is None:
                self.obs = self._first_obs()                                     # (the first step resets every environment, the draw comes after it)
            random_progress(progress, max_len, self.seed)
        for _ in range(int(num_iterations)):
            self.collect()
            mean_reward, done_rate = self.storage.rewards.mean(), self.storage.dones.mean()
            value_loss, surrogate = self.alg.update(self.storage)
            self._scalars = torch.stack((mean_reward, done_rate, value_loss, surrogate, self.actor_critic.std.detach().mean())).double()
            self.iteration += 1
            self.infos.append(dict(iter=self.iteration, **_read_riders(self._riders)))
        return self.infos

    def evaluate(self, num_ticks, groups=None, num_groups=1):
        """The reference's ``cfg.test`` loop: ``num_ticks`` of ``act_inference`` (the mean action) and ``env.step`` on the trainer's environment,
        with no storage write and no update, counted by a fresh ``EpisodeStats`` (``groups`` / ``num_groups``: e.g. the robot type of each
        environment); one host read at the end.  Returns the overall totals -- ``episodes``, ``time_outs``, ``terminations`` (episodes minus
        time-outs: on the toy plant, falls), ``mean_return``, ``mean_length`` -- and the same per group under ``groups``.  ``tick`` and the noise
        sequence are untouched; the training statistics drop the episodes under way (``restart``), which the evaluation has cut in two.  An environment's
        ``episode_terms`` has ``curriculum_enabled`` cleared for the loop: the command ranges stay where training left them."""
        stats = EpisodeStats(self.env.num_envs, groups=groups, num_groups=num_groups, device=self.device)
        if self.obs is None:
            self.obs = self._first_obs()
        terms = self.episode_terms
        enabled = terms.curriculum_enabled if terms is not None else None
        if terms is not None:                                                    # an evaluation does not move the command ranges
            terms.curriculum_enabled = False
        try:
            with torch.no_grad():
                for _ in range(int(num_ticks)):                                  # the actor's memory alone, from zero state where an episode starts
                    action = self.actor_critic.act_inference(self.obs, reset=self._prev_reset)
                    returned, rew, reset, extras = self.env.step(action)
                    if self.storage.hidden is not None:
                        self._prev_reset = reset
                    self.obs = self._rows.read(returned, update=False)           # the statistics stay as training left them
                    stats.add(rew, reset, extras["time_outs"])
                if self._critic_rows is not None:                                # the critic's rows that go with self.obs, for the next collection
                    self.critic_obs = self._critic_rows.read(None, update=False)
        finally:
            if terms is not None:
                terms.curriculum_enabled = enabled
        out = stats.read()
        self.actor_critic.reset_memory()                                         # the critic's memory has not seen these ticks: both start the next collection from zero
        self._prev_reset = None
        self.episode_stats.restart()
        keys = ("episodes", "time_outs", "terminations", "mean_return", "mean_length")
        result = {k: out[k] for k in keys}
        result["groups"] = [{k: g[k] for k in keys} for g in out["groups"]]
        return result

    def save(self, path):
        """The checkpoint as rsl_rl writes it; ``WeightPolicy.from_state_dict(torch.load(path)["model_state_dict"])`` loads its actor.  A recurrent
        trainer's checkpoint loads through the same call as a ``RecurrentWeightPolicy`` (``memory_a`` and the actor; ``step(obs, reset=)``).  With
        normalisation on it also carries ``obs_norm_state_dict`` (rsl_rl 2.x's key), and the actor expects normalised observations:
        ``obs_norm.fold_normalizer(ck["model_state_dict"], ck["obs_norm_state_dict"])`` gives the state dict for raw ones.  With privileged observations as well it carries ``critic_obs_norm_state_dict``, the statistics of the critic's
        rows (``fold_normalizer(..., critic_obs_norm_state_dict=)``); ``load`` refuses a checkpoint whose critic reads rows of another width.  On an environment with
        ``episode_terms`` it carries ``episode_terms_state_dict`` (the x command range, the widenings, the tick), which ``load`` restores when present.
        On an environment with ``plant_rand`` it carries ``plant_rand_state_dict`` (every robot's plant record and draw counter), which ``load``
        restores when present; a checkpoint without it leaves the record as the task made it.  On an environment with ``friction`` it carries
        ``friction_state_dict`` (every robot's friction coefficient and draw counter); ``load`` refuses, before anything is loaded, a checkpoint
        with it on an environment without and a checkpoint without it on an environment with."""
        ck = {"model_state_dict": self.actor_critic.state_dict(), "optimizer_state_dict": self.alg.optimizer.state_dict(), "iter": self.iteration,
              "infos": self.infos}
        _save_parts(_checkpoint_parts(self), ck)
        torch.save(ck, path)

    def load(self, path, load_optimizer=True):
        ck = torch.load(path, map_location=self.device)
        ck_recurrent = any(k.startswith("memory_a.") for k in ck["model_state_dict"])
        if ck_recurrent != (self.recurrent is not None):
            raise ValueError("the checkpoint holds a recurrent actor-critic (memory_a / memory_c) and this trainer is feed-forward" if ck_recurrent else
                             "the checkpoint holds a feed-forward actor-critic and this trainer is recurrent (recurrent=)")
        width = int(ck["model_state_dict"]["critic.0.weight"].shape[1])
        if width != self.actor_critic.critic_width:
            raise ValueError(f"the checkpoint's critic reads rows of {width} columns, this trainer's critic rows of {self.actor_critic.critic_width}")
        _load_parts(_checkpoint_parts(self), ck)
        self.actor_critic.load_state_dict(ck["model_state_dict"])      # (in place: the kernels keep reading the same addresses)
        self.actor_critic.reset_memory()                                         # (a state the loaded memories did not compute)
        self._prev_reset = None
        if load_optimizer:
            self.alg.optimizer.load_state_dict(ck["optimizer_state_dict"])
            if self.alg.device_update:                                           # the device's copy of the learning rate follows the checkpoint's
                self.alg.set_learning_rate(self.alg.optimizer.param_groups[0]["lr"])
        self.iteration = ck["iter"]
        self.infos = list(ck["infos"]) if ck.get("infos") else []
        return ck["infos"]

    def get_inference_policy(self):
        """obs [n, num_obs] -> the actor's mean [n, 12] (``ActorCritic.act_inference``; with normalisation on, of the observation normalised with
        the statistics as they are, without updating them).  A recurrent trainer's policy also takes ``reset=``, the task's reset tensor of the tick
        before, and advances the actor's memory on every call."""
        if self.obs_norm is None:
            return self.actor_critic.act_inference
        return lambda obs, reset=None: self.actor_critic.act_inference(self.obs_norm(obs, update=False), reset=reset)

