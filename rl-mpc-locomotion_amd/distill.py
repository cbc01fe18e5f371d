"""Teacher-student policy distillation on the device (RMA, legged_gym's descendants, rsl_rl 2.x's ``Distillation`` / ``StudentTeacher``; rsl_rl 2.x is
not the reference's version, so the formulas here are the contract).

The randomised task hides what decides a robot's fate from the actor: payload, motor strength, gravity, friction, the terrain beyond the scan, the
noise.  The critic alone sees the truth, in ``env.privileged_obs_buf``.  The standard way to cope, besides a memory in front of the actor, is

    env = BatchedRLTask(..., privileged_obs=PrivilegedObs(n))
    teacher = PPOTrainer(TeacherEnv(env))            # 1. an actor that READS the privileged row, trained with what exists
    teacher.learn(k); teacher.save("teacher.pt")
    d = Distiller(env, "teacher.pt", update="hip")   # 2. a student that reads what the robot has, labelled with the teacher's actions
    d.learn(k); d.save("student.pt")
    tuned = PPOTrainer(env); tuned.load("student.pt", load_optimizer=False); tuned.learn(k)      # 3. PPO fine-tuning of the student

* ``TeacherEnv`` is a view of the task whose observation is the privileged row; ``PPOTrainer`` is unchanged.
* The collection is ONE launch per tick (``act_distill``: ``mpc_ac_act_distill``, include/mpc_ppo.h): the student's actor samples the action the
  task steps with, and beside it the teacher's actor writes its mean, the label, into slot t of the storage.
* ``Distillation.update`` is behaviour cloning of the labels into the student's ACTOR: ``backend="torch"`` is autograd and ``torch.optim.Adam`` over
  ``student.actor.parameters()``; ``backend="hip"`` is the device update (include/mpc_ppo_update.h: ``mpc_ppo_update_grads_distill``,
  ``mpc_ppo_update_apply_actor``) on the same parameters, ``.grad`` tensors and optimiser moments, with no host read per mini-batch.  Neither writes the
  student's critic or ``std``.

Not built: a recurrent student or teacher, DAgger's mixing of teacher actions into the rollout, normalising the student's observations during
distillation, initialising the student's critic from the teacher's, a bf16 path."""
import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import need_gpu, tensor_arg
from .episode import EpisodeStats
from .ppo import (NUM_ACTIONS, ActorCritic, PPOConfig, _checkpoint_parts, _load_parts, _read_riders, _Rider, _save_parts, check, episode_record, lib,
                  update_lib)

LOSS_TYPES = {"mse": 0, "huber": 1}                # mpc_ppo_update_grads_distill's loss_type; huber's delta is 1
BACKENDS = ("torch", "hip")


class TeacherEnv:
    """A view of a ``BatchedRLTask`` made with ``privileged_obs=`` whose observation IS the privileged row: ``num_obs`` is ``env.num_privileged_obs``,
    ``reset()`` and ``step()`` return ``env.privileged_obs_buf`` -- the task's own buffer, nothing is copied (the trainer keeps slot t's row before
    the next step rewrites it) -- and every other attribute, read or written, is the task's.  ``PPOTrainer(TeacherEnv(env))`` then trains an actor on
    privileged rows with no change of its own."""

    def __init__(self, env):
        if getattr(env, "num_privileged_obs", None) is None:
            raise ValueError("TeacherEnv: the task has no privileged observations (BatchedRLTask(privileged_obs=))")
        object.__setattr__(self, "_env", env)

    @property
    def num_obs(self):
        return self._env.num_privileged_obs

    def reset(self):
        self._env.reset()
        return self._env.privileged_obs_buf

    def step(self, actions, **kw):
        _, rew, reset, extras = self._env.step(actions, **kw)
        return self._env.privileged_obs_buf, rew, reset, extras

    def __getattr__(self, name):                   # (only what the view does not define itself)
        return getattr(self._env, name)

    def __setattr__(self, name, value):
        setattr(self._env, name, value)


@dataclass
class DistillConfig:
    num_steps_per_env: int = 24                    # per iteration
    num_learning_epochs: int = 5
    num_mini_batches: int = 4                      # mini-batch size = num_envs * num_steps_per_env / num_mini_batches
    learning_rate: float = 1.0e-3                  # fixed: there is no kl to adapt to
    max_grad_norm: float = 1.0
    loss_type: str = "mse"                         # or "huber" (delta = 1)
    student_noise_std: float = 0.1                 # fills the student's std, which distillation never trains
    actor_hidden_dims: tuple = PPOConfig.actor_hidden_dims
    critic_hidden_dims: tuple = PPOConfig.critic_hidden_dims


class DistillStorage:
    """What a distillation iteration keeps: [T, N, ...] float32 ``observations`` [T,N,W] (the student's rows), ``actions`` (what the student
    sampled), ``mu``, ``sigma`` and ``teacher_actions`` [T,N,12] (the labels), ``dones`` [T,N,1].  ``act_distill`` writes into ``slot(t)``."""

    def __init__(self, n, T, device, num_obs):
        self.n, self.T, self.device = int(n), int(T), torch.device(device)
        z = lambda k: torch.zeros((self.T, self.n, k), dtype=torch.float32, device=self.device)
        self.observations, self.actions, self.mu, self.sigma, self.teacher_actions, self.dones = (z(num_obs), z(NUM_ACTIONS), z(NUM_ACTIONS), z(NUM_ACTIONS),
                                                                                                  z(NUM_ACTIONS), z(1))

    def slot(self, t):
        return dict(actions=self.actions[t], mu=self.mu[t], sigma=self.sigma[t], teacher_actions=self.teacher_actions[t])

    def indices(self, num_mini_batches):
        """(the permutation, the mini-batch size): ``RolloutStorage.mini_batch_generator``'s one draw, ``torch.randperm`` over
        num_mini_batches * (T N // num_mini_batches) on the storage's device, so both backends consume the same indices from torch's generator."""
        size = self.n * self.T // num_mini_batches
        if size < 1:
            raise ValueError("fewer rows than mini-batches")
        return torch.randperm(num_mini_batches * size, device=self.device), size

    def mini_batch_generator(self, num_mini_batches, num_epochs=5, indices=None):
        """Index slices into the flat T N rows: the same ``num_mini_batches`` slices of one permutation in every epoch, as rsl_rl's generator takes them."""
        size = self.n * self.T // num_mini_batches
        idx = self.indices(num_mini_batches)[0] if indices is None else indices
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                yield idx[i * size:(i + 1) * size]


def act_distill(student, teacher, obs, teacher_obs, seed, step, out=None, return_eps=False):
    """The collection launch of distillation: obs [n, student.num_obs] -> the student's ``actions``, ``mu``, ``sigma`` [n,12] (bit for bit those of
    ``student.act`` with the same seed and step; and ``eps`` if asked), teacher_obs [n, teacher.num_obs] -> ``teacher_actions`` [n,12] (bit for bit
    ``teacher.act_inference``), in ONE launch.  ``out``: the same dict of caller's tensors (``DistillStorage.slot(t)``)."""
    n = student._ready("act_distill", obs)
    if teacher._ready("act_distill", teacher_obs) != n:
        raise ValueError("act_distill: obs and teacher_obs hold different numbers of rows")
    dev = obs.device
    keys = ("actions", "mu", "sigma", "teacher_actions")
    if out is None:
        out = {k: torch.empty((n, NUM_ACTIONS), dtype=torch.float32, device=dev) for k in keys}
    else:
        for k in keys:
            tensor_arg(out[k], torch.float32, n * NUM_ACTIONS, k)
    eps = torch.empty((n, NUM_ACTIONS), dtype=torch.float32, device=dev) if return_eps else None
    check(lib().mpc_ac_act_distill(student._handle, teacher._handle, n, obs.data_ptr(), teacher_obs.data_ptr(), int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF,
                                   out["actions"].data_ptr(), out["mu"].data_ptr(), out["sigma"].data_ptr(), out["teacher_actions"].data_ptr(),
                                   eps.data_ptr() if return_eps else None, _lib.stream(dev)), "mpc_ac_act_distill")
    return dict(out, eps=eps) if return_eps else out


class Distillation:
    """Behaviour cloning of ``storage.teacher_actions`` into ``student.actor``: per mini-batch the loss (``mse`` or ``huber`` with delta 1, mean over
    the rows and the twelve actions) of the actor's mean, ``clip_grad_norm_`` and one Adam step over ``student.actor.parameters()``.  The critic's
    parameters and ``std``, their ``.grad`` and (if another optimiser keeps some) their moments are never written.

    ``backend="torch"``: autograd, on whatever device the storage lives on.  ``backend="hip"``: include/mpc_ppo_update.h's distillation entry
    points on the parameters, ``.grad`` tensors and moments where torch keeps them -- ``optimizer.state_dict()`` stays the checkpoint and moves between
    the backends -- with no host read."""

    def __init__(self, student, cfg=None, backend="torch"):
        self.cfg = cfg if cfg is not None else DistillConfig()
        if backend not in BACKENDS:
            raise ValueError("backend is 'torch' or 'hip'")
        if self.cfg.loss_type not in LOSS_TYPES:
            raise ValueError(f"loss_type is 'mse' or 'huber', not {self.cfg.loss_type!r}")
        if getattr(student, "is_recurrent", False):
            raise ValueError("a recurrent student is not built")
        self.student, self.backend = student, backend
        self.learning_rate = float(self.cfg.learning_rate)
        self.optimizer = torch.optim.Adam(student.actor.parameters(), lr=self.learning_rate)
        self.last_terms = None
        self._handle, self._max_rows, self._bound, self._storage_ptrs, self._ac_ptrs, self._unused, self.lr_device = None, 0, None, None, None, None, None
        if backend == "hip":
            need_gpu('Distillation(backend="hip")', student.std)
            update_lib()
            self.lr_device = torch.full((1,), self.learning_rate, dtype=torch.float64, device=student.std.device)

    __del__ = _lib.finalizer("mpc_ppo_update_destroy")

    def actor_params(self):
        """The actor's tensors in ``mpc_ac_bind``'s order (weights, then biases): the head of ``student.bind_order()``."""
        return self.student.bind_order()[:2 * len(self.student._linears(self.student.actor))]

    # ---- torch ----------------------------------------------------------------------------------------------------------------------------
    def loss(self, mu, target):
        f = torch.nn.functional.mse_loss if self.cfg.loss_type == "mse" else torch.nn.functional.huber_loss
        return f(mu, target)

    def _update_torch(self, storage, indices):
        c = self.cfg
        obs, target = storage.observations.flatten(0, 1), storage.teacher_actions.flatten(0, 1)
        mean_loss, mean_gap, k = 0.0, 0.0, 0
        for b in storage.mini_batch_generator(c.num_mini_batches, c.num_learning_epochs, indices):
            mu = self.student.actor(obs[b])
            loss = self.loss(mu, target[b])
            self.optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(self.student.actor.parameters(), c.max_grad_norm)
            self.optimizer.step()
            gap = (mu.detach() - target[b]).abs().mean()
            self.last_terms = (loss.detach(), gap)
            mean_loss, mean_gap, k = mean_loss + loss.detach(), mean_gap + gap, k + 1
        return mean_loss / k, mean_gap / k

    # ---- the device update ----------------------------------------------------------------------------------------------------------------------
    def _device_state(self, rows):
        """The handle over the student's ``mpc_ac``, sized for ``rows`` and bound to the current addresses of the actor's gradients and moments (created
        here, on the first step, as torch creates them); returns the actor's common step count.  The handle's bind takes a pointer for every tensor of
        the ``mpc_ac``: the critic's and std's slots get ``_unused``, a buffer that the distillation entry points never touch."""
        ac = self.student
        dev = ac.std.device
        ac._ready("Distillation.update", torch.empty((1, ac.num_obs), dtype=torch.float32, device=dev))      # (the handle and its binding: nothing is launched)
        params, actor = ac.bind_order(), self.actor_params()
        steps = set()
        for p in actor:
            st = self.optimizer.state[p]
            if len(st) == 0:                                                      # torch.optim.Adam._init_group
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif st["step"].is_cuda:
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
        rest = params[len(actor):]
        if self._unused is None or self._unused.device != dev:
            self._unused = torch.zeros(max(p.numel() for p in rest), dtype=torch.float32, device=dev)
        tensors = [p.grad for p in actor] + [self.optimizer.state[p][key] for key in ("exp_avg", "exp_avg_sq") for p in actor]
        ptrs = _lib.addresses_to_bind(tensors, self._bound, dev, "gradients and Adam's moments must be contiguous float32 tensors shaped like their parameters, on their device",
                                      like=3 * actor)
        if ptrs is not None:
            n, arr, pad = len(actor), _lib.ptr_array, [self._unused.data_ptr()] * len(rest)
            check(update_lib().mpc_ppo_update_bind(self._handle, arr(list(ptrs[:n]) + pad), arr(list(ptrs[n:2 * n]) + pad), arr(list(ptrs[2 * n:]) + pad)),
                  "mpc_ppo_update_bind")
            self._bound = ptrs
        return steps.pop()

    def _bind_storage(self, storage):
        """The storage's rows and the labels on the handle (after ``_device_state``), where their addresses have changed.  The distillation calls read
        ``d_obs`` and the targets alone; ``mpc_ppo_update_set_storage`` wants every pointer, so the four per-row scalars' slots get ``dones``."""
        L, total = update_lib(), storage.n * storage.T
        wide = lambda t, name: tensor_arg(t, torch.float32, total * NUM_ACTIONS, name).data_ptr()
        obs = tensor_arg(storage.observations, torch.float32, total * self.student.num_obs, "storage.observations").data_ptr()
        actions, mu, sigma, target = (wide(getattr(storage, k), "storage." + k) for k in ("actions", "mu", "sigma", "teacher_actions"))
        flag = tensor_arg(storage.dones, torch.float32, total, "storage.dones").data_ptr()
        ptrs = (obs, actions, mu, sigma, target, flag)
        if ptrs != self._storage_ptrs:
            check(L.mpc_ppo_update_set_storage(self._handle, total, obs, actions, flag, flag, flag, flag, mu, sigma), "mpc_ppo_update_set_storage")
            check(L.mpc_ppo_update_set_distill_targets(self._handle, target), "mpc_ppo_update_set_distill_targets")
            self._storage_ptrs = ptrs

    def _update_hip(self, storage, indices):
        c, ac = self.cfg, self.student
        dev = ac.std.device
        need_gpu("Distillation.update", storage.observations, ac.std)
        if storage.device != dev:
            raise _lib.MpcLibraryError("Distillation.update: the storage and the parameters live on different devices")
        total = storage.n * storage.T
        if indices is None:
            indices, size = storage.indices(c.num_mini_batches)
        else:
            size = total // c.num_mini_batches
        tensor_arg(indices, torch.long, c.num_mini_batches * size, "indices")
        step = self._device_state(size)
        L = update_lib()
        self._bind_storage(storage)
        group = self.optimizer.param_groups[0]
        beta1, beta2 = group["betas"]
        if group["amsgrad"] or group["weight_decay"] != 0 or group["maximize"]:
            raise ValueError("the device update restates plain Adam: no amsgrad, weight decay or maximize")
        k = c.num_learning_epochs * c.num_mini_batches
        terms = torch.empty((k, 2), dtype=torch.float32, device=dev)
        stream = _lib.stream(dev)
        loss_type = LOSS_TYPES[c.loss_type]
        with torch.cuda.device(dev):
            for e in range(c.num_learning_epochs):
                for i in range(c.num_mini_batches):
                    j = e * c.num_mini_batches + i
                    check(L.mpc_ppo_update_grads_distill(self._handle, size, indices.data_ptr() + 8 * i * size, loss_type, terms[j].data_ptr(), stream),
                          "mpc_ppo_update_grads_distill")
                    step += 1
                    check(L.mpc_ppo_update_apply_actor(self._handle, float(c.max_grad_norm), float(beta1), float(beta2), float(group["eps"]), step,
                                                       self.lr_device.data_ptr(), stream), "mpc_ppo_update_apply_actor")
        for p in self.actor_params():
            self.optimizer.state[p]["step"] += float(k)                          # (host tensors: no device work)
        self.last_terms = (terms[k - 1, 0], terms[k - 1, 1])
        return terms[:, 0].mean(), terms[:, 1].mean()

    def update(self, storage, indices=None):
        """One update over the storage: num_learning_epochs x num_mini_batches Adam steps on the actor.  Returns device tensors (mean behaviour loss,
        mean |mu - teacher action|) over the mini-batches.  ``indices`` (for tests) replaces the ``torch.randperm``."""
        return self._update_hip(storage, indices) if self.backend == "hip" else self._update_torch(storage, indices)


def _hidden_dims(sd, net):
    """The hidden widths of ``net`` ('actor' or 'critic') in an rsl_rl state dict: every ``Linear`` but the last."""
    layers = sorted(int(k.split(".")[1]) for k in sd if k.startswith(net + ".") and k.endswith(".weight"))
    return tuple(int(sd[f"{net}.{l}.weight"].shape[0]) for l in layers[:-1])


def load_teacher(teacher, num_privileged_obs, obs_norm_eps=1e-2):
    """``teacher`` -- a checkpoint path, a checkpoint dict (``model_state_dict`` and what ``PPOTrainer.save`` puts beside it), a bare model state dict
    or an ``ActorCritic`` -- as a frozen ``ActorCritic`` on the CPU whose actor reads RAW privileged rows of ``num_privileged_obs`` columns: a
    checkpoint carrying ``obs_norm_state_dict`` is folded into the first layers (``obs_norm.fold_normalizer``, ``obs_norm_eps`` the normaliser's).
    An ``ActorCritic`` is taken as it is, where it is.  ValueError for a recurrent teacher and for an actor of another width."""
    if isinstance(teacher, ActorCritic) or getattr(teacher, "is_recurrent", False):
        if getattr(teacher, "is_recurrent", False):
            raise ValueError("a recurrent teacher is not built")
        width = teacher.num_obs
        net = teacher
    else:
        ck = torch.load(teacher, map_location="cpu") if isinstance(teacher, (str, bytes)) or hasattr(teacher, "__fspath__") else teacher
        sd = ck["model_state_dict"] if "model_state_dict" in ck else ck
        if any(k.startswith("memory_a.") for k in sd):
            raise ValueError("the teacher's checkpoint holds a recurrent actor-critic (memory_a / memory_c): a recurrent teacher is not built")
        if ck is not sd and "obs_norm_state_dict" in ck:
            from .obs_norm import fold_normalizer
            sd = fold_normalizer(sd, ck["obs_norm_state_dict"], eps=obs_norm_eps, critic_obs_norm_state_dict=ck.get("critic_obs_norm_state_dict"))
        width, net = int(sd["actor.0.weight"].shape[1]), None
    if width != int(num_privileged_obs):
        raise ValueError(f"the teacher's actor reads rows of {width} columns, the task's privileged rows have {int(num_privileged_obs)}")
    if net is None:
        critic_width = int(sd["critic.0.weight"].shape[1])
        net = ActorCritic(width, NUM_ACTIONS, _hidden_dims(sd, "actor"), _hidden_dims(sd, "critic"), num_critic_obs=None if critic_width == width else critic_width)
        net.load_state_dict({k: v.detach().cpu() for k, v in sd.items()})
    for p in net.parameters():                                                   # frozen: nothing here ever writes it
        p.requires_grad_(False)
    return net


class Distiller:
    """The runner of the second stage: ``env`` is a task with ``privileged_obs``, ``teacher`` what ``load_teacher`` takes (its actor reads
    ``env.privileged_obs_buf``).  The student is ``ActorCritic(env.num_obs, ..., num_critic_obs=env.num_privileged_obs)`` -- the shape ``PPOTrainer(env)``
    builds, so ``PPOTrainer(env).load(path, load_optimizer=False)`` takes the distilled checkpoint for fine-tuning and
    ``WeightPolicy.from_state_dict`` deploys it; its critic stays as initialised and its ``std`` is ``cfg.student_noise_std``.

    An iteration: T times ``act_distill`` into slot t (the student samples, the teacher labels, one launch), ``env.step`` with the student's action;
    then ``Distillation.update``; then the one host read, which yields the record: ``iter``, ``behavior_loss``, ``action_gap`` (mean |mu - teacher
    action|), ``mean_reward`` and the episode statistics' entries.  Every refusal comes before the device is asked for."""

    def __init__(self, env, teacher, cfg=None, seed=1, update="torch", device=None, teacher_obs_norm_eps=1e-2):
        self.cfg = cfg if cfg is not None else DistillConfig()
        if update not in BACKENDS:
            raise ValueError("update is 'torch' or 'hip'")
        if self.cfg.loss_type not in LOSS_TYPES:
            raise ValueError(f"loss_type is 'mse' or 'huber', not {self.cfg.loss_type!r}")
        priv = getattr(env, "num_privileged_obs", None)
        if priv is None:
            raise ValueError("Distiller: the task has no privileged observations (BatchedRLTask(privileged_obs=)), which the teacher reads")
        teacher = load_teacher(teacher, priv, teacher_obs_norm_eps)
        need_gpu("Distiller")
        c = self.cfg
        self.env, self.seed = env, int(seed)
        self.device = _lib.device_of(device if device is not None else getattr(env, "device", None))
        torch.manual_seed(self.seed)
        self.teacher = teacher.to(self.device)
        self.actor_critic = ActorCritic(env.num_obs, env.num_actions, c.actor_hidden_dims, c.critic_hidden_dims, init_noise_std=c.student_noise_std,
                                        num_critic_obs=priv).to(self.device)
        self.alg = Distillation(self.actor_critic, c, backend=update)
        self.storage = DistillStorage(env.num_envs, c.num_steps_per_env, self.device, env.num_obs)
        self.episode_stats = EpisodeStats(env.num_envs, device=self.device)
        self.iteration, self.tick, self.obs, self.infos = 0, 0, None, []
        # what PPOTrainer's checkpoint parts look for: the distilled checkpoint carries what a fine-tuning trainer on this task refuses to go without
        self.obs_norm = self.critic_obs_norm = None
        self.episode_terms, self.plant_rand, self.friction = (getattr(env, name, None) for name in ("episode_terms", "plant_rand", "friction"))
        self._scalars = None
        self._riders = [_Rider(lambda: self._scalars, lambda values: dict(zip(("behavior_loss", "action_gap", "mean_reward"), values))),
                        _Rider(lambda: self.episode_stats.summary, episode_record)]

    def collect(self):
        """T ticks, entirely on the device; returns the mean reward of the T N steps as a device tensor."""
        st, env = self.storage, self.env
        if self.obs is None:
            self.obs = env.reset()
        reward = torch.zeros((), dtype=torch.float32, device=self.device)
        with torch.no_grad():
            for t in range(st.T):
                act_distill(self.actor_critic, self.teacher, self.obs, env.privileged_obs_buf, self.seed, self.tick, out=st.slot(t))
                st.observations[t].copy_(self.obs)
                self.obs, rew, reset, extras = env.step(st.actions[t])
                st.dones[t, :, 0].copy_(reset)
                reward += rew.mean()
                self.episode_stats.add(rew, reset, extras["time_outs"])
                self.tick += 1
        return reward / st.T

    def learn(self, num_iterations):
        """``num_iterations`` of collection + update; appends one record per iteration to ``infos`` (one host read each, after the update) and returns
        the list."""
        for _ in range(int(num_iterations)):
            mean_reward = self.collect()
            loss, gap = self.alg.update(self.storage)
            self._scalars = torch.stack((loss, gap, mean_reward)).double()
            self.iteration += 1
            self.infos.append(dict(iter=self.iteration, **_read_riders(self._riders)))
        return self.infos

    def save(self, path):
        """rsl_rl's checkpoint keys, as ``PPOTrainer.save`` writes them (the optimiser's is Adam over the actor's parameters)."""
        ck = {"model_state_dict": self.actor_critic.state_dict(), "optimizer_state_dict": self.alg.optimizer.state_dict(), "iter": self.iteration,
              "infos": self.infos}
        _save_parts(_checkpoint_parts(self), ck)
        torch.save(ck, path)

    def load(self, path, load_optimizer=True):
        ck = torch.load(path, map_location=self.device)
        sd = ck["model_state_dict"]
        if any(k.startswith("memory_a.") for k in sd):
            raise ValueError("the checkpoint holds a recurrent actor-critic and the student is feed-forward")
        for net, width in (("actor", self.actor_critic.num_obs), ("critic", self.actor_critic.critic_width)):
            if int(sd[f"{net}.0.weight"].shape[1]) != width:
                raise ValueError(f"the checkpoint's {net} reads rows of {int(sd[f'{net}.0.weight'].shape[1])} columns, the student's rows of {width}")
        _load_parts(_checkpoint_parts(self), ck)
        self.actor_critic.load_state_dict(sd)                                    # (in place: the kernels keep reading the same addresses)
        if load_optimizer:
            self.alg.optimizer.load_state_dict(ck["optimizer_state_dict"])
        self.iteration = ck["iter"]
        self.infos = list(ck["infos"]) if ck.get("infos") else []
        return ck["infos"]

    def get_inference_policy(self):
        """obs [n, num_obs] -> the student's mean [n, 12] (``ActorCritic.act_inference``)."""
        return self.actor_critic.act_inference
