"""Batched weight policy: observations -> actor MLP -> MPC weights, on the GPU.

Host-side mirror of the reference's ``WeightPolicy`` (RL_Environment/WeightPolicy.py:33-139) for N robots at once:
``compute_observations`` + ``step`` keep their meaning, tensors replace the per-robot numpy arrays.  The network is the
actor of rsl_rl's ActorCritic (Linear/ELU stack 48-512-256-128-12, RL_Environment/tasks/legged_config_ppo.py:5-9);
``from_state_dict`` takes the ``model_state_dict`` of a checkpoint exactly as ``WeightPolicy.__init__`` loads it (:75-77).

``RecurrentWeightPolicy`` is the same controller-side object for a recurrent actor (``recurrent.ActorCriticRecurrent``: rsl_rl's ``memory_a``, one LSTM
layer, in front of the actor's MLP): ``step`` is ONE launch (csrc/mpc_recurrent_policy.h, csrc/recurrent_policy.h) that advances the memory, runs the
actor on h' and maps the actions to MPC weights; the state ``h``, ``c`` [n, H] lives on the device and ``reset`` flags zero a robot's memory inside
the step.  ``WeightPolicy.from_state_dict`` returns one for a ``model_state_dict`` that has ``memory_a.*`` keys.
"""
import ctypes as C

import numpy as np

from . import _lib

MPC_PARAM_SCALE = (4, 4, 4, 20, 20, 20, 1, 1, 1, 1, 1, 1)     # MPC_Controller/Parameters.py:25-28
MPC_PARAM_CONST = (5, 5, 5, 50, 50, 50, 1, 1, 1, 1, 1, 1)     # MPC_Controller/Parameters.py:30-33


def _array(t):
    """A state dict's value (a torch tensor on any device, or an array) as float32 numpy."""
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)


def actor_layers(state_dict):
    """[(weight, bias), ...] of the ``actor.*`` Linear layers of a ``model_state_dict``, in order, float32 numpy."""
    idx = sorted({int(k.split(".")[1]) for k in state_dict if k.startswith("actor.") and k.endswith(".weight")})
    return [(_array(state_dict[f"actor.{i}.weight"]), _array(state_dict[f"actor.{i}.bias"])) for i in idx]


def is_recurrent(state_dict):
    return any(k.startswith("memory_a.") for k in state_dict)


LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def recurrent_policy_params(state_dict):
    """What a deployed recurrent actor is made of, from the ``model_state_dict`` of a recurrent checkpoint (rsl_rl's ``ActorCriticRecurrent`` keys):
    ``(lstm, layers)`` with ``lstm = (w_ih [4H, I], w_hh [4H, H], b_ih [4H], b_hh [4H])`` from ``memory_a.rnn.*_l0`` and ``layers`` the ``actor.*``
    Linear stack, float32 numpy.  ``memory_c.*``, ``critic.*`` and ``std`` are ignored.  Pure: runs on the CPU, touches no device.

    ValueError for a dict without ``memory_a.*``, for any ``*_l1`` key (stacked layers are not built), for a ``weight_ih_l0`` whose row count is not
    4 H (a GRU's is 3 H: not built), and for an ``actor.0.weight`` that does not read H inputs."""
    if not is_recurrent(state_dict):
        raise ValueError("not a recurrent checkpoint: the state dict has no memory_a.* keys")
    stacked = sorted(k for k in state_dict if k.startswith("memory_") and k.endswith("_l1"))
    if stacked:
        raise ValueError(f"stacked recurrent layers are not built: the state dict has {stacked[0]}")
    missing = [k for k in LSTM_KEYS if f"memory_a.rnn.{k}" not in state_dict]
    if missing:
        raise ValueError(f"memory_a.rnn.{missing[0]} is missing")
    w_ih, w_hh, b_ih, b_hh = (_array(state_dict[f"memory_a.rnn.{k}"]) for k in LSTM_KEYS)
    if w_hh.ndim != 2 or w_ih.ndim != 2:
        raise ValueError("memory_a.rnn.weight_ih_l0 and weight_hh_l0 must be matrices")
    H = w_hh.shape[1]
    if w_ih.shape[0] != 4 * H:
        raise ValueError(f"memory_a.rnn.weight_ih_l0 has {w_ih.shape[0]} rows for a state of {H}: an LSTM has 4 H = {4 * H} (a GRU's 3 H is not built)")
    if w_hh.shape[0] != 4 * H or b_ih.shape != (4 * H,) or b_hh.shape != (4 * H,):
        raise ValueError(f"memory_a.rnn: weight_hh_l0 must be ({4 * H}, {H}) and the biases ({4 * H},)")
    layers = actor_layers(state_dict)
    if not layers:
        raise ValueError("the state dict has no actor.* layers")
    if layers[0][0].shape[1] != H:
        raise ValueError(f"actor.0.weight reads {layers[0][0].shape[1]} inputs, memory_a gives {H}")
    return (w_ih, w_hh, b_ih, b_hh), layers


def _checked_layers(layers):
    ws = [np.ascontiguousarray(w, dtype=np.float32) for w, _ in layers]
    bs = [np.ascontiguousarray(b, dtype=np.float32) for _, b in layers]
    dims = [ws[0].shape[1]] + [w.shape[0] for w in ws]
    for l, (w, b) in enumerate(zip(ws, bs)):
        if w.shape != (dims[l + 1], dims[l]) or b.shape != (dims[l + 1],):
            raise ValueError(f"layer {l}: expected weight {(dims[l + 1], dims[l])} and bias {(dims[l + 1],)}")
    return ws, bs, dims


class _ControllerSide:
    """What a weight policy does around its network, whatever the network is: the observation kernels and the command record.  Needs ``device``,
    ``num_obs`` and ``_scales`` (the four observation scales, float32 numpy)."""

    def compute_observations(self, dof_states, est, ground_normal_yaw, commands, actions):
        """dof_states [n,12,2], est [n,18] (vBody, omegaBody, rpy, R), ground_normal_yaw [n,3], commands [n,3],
        actions [n,12] (previous policy output) -> obs [n,48]."""
        import torch
        n = commands.shape[0]
        for name, t, k in (("dof_states", dof_states, 24), ("est", est, 18), ("ground_normal_yaw", ground_normal_yaw, 3),
                           ("commands", commands, 3), ("actions", actions, 12)):
            _lib.tensor_arg(t, torch.float32, n * k, name)
        obs = torch.empty((n, 48), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().mpc_policy_observations(n, dof_states.data_ptr(), est.data_ptr(), ground_normal_yaw.data_ptr(), commands.data_ptr(),
                                                      actions.data_ptr(), self._scales.ctypes.data, obs.data_ptr(), _lib.stream(self.device)),
                   "mpc_policy_observations")
        return obs

    def observations_from(self, ctl, dof_states, commands, actions):
        """compute_observations with the StateEstimate taken where the controller keeps it (``ctl``: a BatchedLocomotion whose
        ``update_estimate`` / ``run`` has just been called): RobotRunnerPolicy.run's ``compute_observations(dof_states, result, commands,
        self.weights)`` (RobotRunnerPolicy.py:72-78) without copying the estimate out first."""
        import torch
        n = ctl.n
        for name, t, k in (("dof_states", dof_states, 24), ("commands", commands, 3), ("actions", actions, 12)):
            _lib.tensor_arg(t, torch.float32, n * k, name)
        obs = torch.empty((n, 48), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().mpc_ctrl_policy_observations(ctl._handle, dof_states.data_ptr(), commands.data_ptr(), actions.data_ptr(), self._scales.ctypes.data,
                                                           obs.data_ptr(), _lib.stream(self.device)), "mpc_ctrl_policy_observations")
        return obs

    def pack_commands(self, commands, weights):
        """[n,3] velocity commands + [n,12] MPC weights -> the [n,16] command record of BatchedLocomotion.run/step."""
        import torch
        n = commands.shape[0]
        _lib.tensor_arg(commands, torch.float32, n * 3, "commands"); _lib.tensor_arg(weights, torch.float32, n * 12, "weights")
        out = torch.empty((n, 16), dtype=torch.float32, device=self.device)
        _lib.check(_lib.lib().mpc_pack_commands(n, commands.data_ptr(), weights.data_ptr(), out.data_ptr(), _lib.stream(self.device)), "mpc_pack_commands")
        return out


class WeightPolicy(_ControllerSide):
    def __init__(self, layers, scale=MPC_PARAM_SCALE, const=MPC_PARAM_CONST, obs_scales=(1.0, 1.0, 1.0, 1.0), device=None):
        """layers: [(weight [out, in], bias [out]), ...] float32 (torch Linear layout).
        obs_scales = (linearVelocityScale, angularVelocityScale, dofPositionScale, dofVelocityScale), cfg/task/*.yaml."""
        import torch
        _lib.need_gpu("WeightPolicy")
        self.device = _lib.device_of(device)
        torch.cuda.set_device(self.device)
        ws, bs, dims = _checked_layers(layers)
        self.dims = dims
        self.num_obs, self.num_actions = dims[0], dims[-1]
        sc = np.ascontiguousarray(scale, dtype=np.float32); ct = np.ascontiguousarray(const, dtype=np.float32)
        if len(sc) != self.num_actions or len(ct) != self.num_actions:
            raise ValueError("scale / const need one entry per action")
        self._scales = np.ascontiguousarray(obs_scales, dtype=np.float32)
        L = len(ws)
        d = (C.c_int * (L + 1))(*dims)
        wp = (C.c_void_p * L)(*[w.ctypes.data for w in ws])
        bp = (C.c_void_p * L)(*[b.ctypes.data for b in bs])
        self._handle = C.c_void_p()
        _lib.check(_lib.lib().mpc_policy_create(C.byref(self._handle), L, C.cast(d, C.c_void_p), C.cast(wp, C.c_void_p),
                                                C.cast(bp, C.c_void_p), sc.ctypes.data, ct.ctypes.data), "mpc_policy_create")

    @classmethod
    def from_state_dict(cls, state_dict, **kw):
        """The policy of a checkpoint's ``model_state_dict``: this class for a feed-forward actor, a ``RecurrentWeightPolicy`` for a recurrent one
        (``memory_a.*`` keys)."""
        if is_recurrent(state_dict):
            return RecurrentWeightPolicy.from_state_dict(state_dict, **kw)
        return cls(actor_layers(state_dict), **kw)

    __del__ = _lib.finalizer("mpc_policy_destroy")

    def step(self, obs, return_actions=False):
        """obs [n, 48] -> MPC weights [n, 12] (and the raw actor output if asked)."""
        import torch
        n = obs.shape[0]
        _lib.tensor_arg(obs, torch.float32, n * self.num_obs, "obs")
        weights = torch.empty((n, self.num_actions), dtype=torch.float32, device=self.device)
        actions = torch.empty_like(weights) if return_actions else None
        _lib.check(_lib.lib().mpc_policy_step(self._handle, n, obs.data_ptr(), actions.data_ptr() if return_actions else None,
                                              weights.data_ptr(), _lib.stream(self.device)), "mpc_policy_step")
        return (weights, actions) if return_actions else weights


# the entry points of csrc/mpc_recurrent_policy.h (bound here, not in _lib.SYMBOLS, which lists include/mpc_batch.h)
RECURRENT_DECLS = {
    "mpc_recurrent_policy_create": (_lib.ci, [_lib.pvp, _lib.ci, _lib.ci, _lib.vp, _lib.vp, _lib.vp, _lib.vp, _lib.ci, _lib.vp, _lib.vp, _lib.vp, _lib.vp, _lib.vp]),
    "mpc_recurrent_policy_destroy": (None, [_lib.vp]),
    "mpc_recurrent_policy_step": (_lib.ci, [_lib.vp, _lib.ci, _lib.vp, _lib.vp, _lib.vp, _lib.vp, _lib.vp, _lib.vp, _lib.vp]),
    "mpc_recurrent_policy_last_error": (_lib.text, []),
}
RECURRENT_SYMBOLS = list(RECURRENT_DECLS)
recurrent_lib = _lib.binder(RECURRENT_DECLS)
recurrent_check = _lib.checker(recurrent_lib, "mpc_recurrent_policy_last_error")


class RecurrentWeightPolicy(_ControllerSide):
    """A deployed recurrent actor: ``memory_a``'s LSTM step, the actor's MLP on h', clamp and the affine map to MPC weights, ONE launch per tick.

    ``h``, ``c`` [n, H] float32 on the device: the memory's state, allocated (zero) on the first ``step`` and again on a new ``n``, as
    ``recurrent.Memory.state`` does, and advanced in place by every ``step``."""

    def __init__(self, lstm, layers, scale=MPC_PARAM_SCALE, const=MPC_PARAM_CONST, obs_scales=(1.0, 1.0, 1.0, 1.0), device=None):
        """lstm = (w_ih [4H, I], w_hh [4H, H], b_ih [4H], b_hh [4H]) float32, torch's nn.LSTM layout (gate rows i, f, g, o); layers, scale, const and
        obs_scales as ``WeightPolicy``'s, the first layer reading H inputs."""
        import torch
        _lib.need_gpu("RecurrentWeightPolicy")
        self.device = _lib.device_of(device)
        torch.cuda.set_device(self.device)
        w_ih, w_hh, b_ih, b_hh = (np.ascontiguousarray(a, dtype=np.float32) for a in lstm)
        if w_hh.ndim != 2 or w_ih.ndim != 2 or w_ih.shape[0] != 4 * w_hh.shape[1]:
            raise ValueError("lstm: expected w_ih [4H, I] and w_hh [4H, H]")
        H, I = w_hh.shape[1], w_ih.shape[1]
        if w_hh.shape[0] != 4 * H or b_ih.shape != (4 * H,) or b_hh.shape != (4 * H,):
            raise ValueError(f"lstm: expected w_hh {(4 * H, H)} and biases {(4 * H,)}")
        ws, bs, dims = _checked_layers(layers)
        if dims[0] != H:
            raise ValueError(f"layer 0 reads {dims[0]} inputs, the memory gives {H}")
        self.dims, self.hidden_size = dims, H
        self.num_obs, self.num_actions = I, dims[-1]
        sc = np.ascontiguousarray(scale, dtype=np.float32); ct = np.ascontiguousarray(const, dtype=np.float32)
        if len(sc) != self.num_actions or len(ct) != self.num_actions:
            raise ValueError("scale / const need one entry per action")
        self._scales = np.ascontiguousarray(obs_scales, dtype=np.float32)
        self.h, self.c = None, None
        L = len(ws)
        d = (C.c_int * (L + 1))(*dims)
        wp = (C.c_void_p * L)(*[w.ctypes.data for w in ws])
        bp = (C.c_void_p * L)(*[b.ctypes.data for b in bs])
        self._handle = C.c_void_p()
        recurrent_check(recurrent_lib().mpc_recurrent_policy_create(C.byref(self._handle), I, H, w_ih.ctypes.data, w_hh.ctypes.data, b_ih.ctypes.data, b_hh.ctypes.data,
                                                                    L, C.cast(d, C.c_void_p), C.cast(wp, C.c_void_p), C.cast(bp, C.c_void_p), sc.ctypes.data,
                                                                    ct.ctypes.data), "mpc_recurrent_policy_create")

    @classmethod
    def from_state_dict(cls, model_state_dict, **kw):
        lstm, layers = recurrent_policy_params(model_state_dict)
        return cls(lstm, layers, **kw)

    __del__ = _lib.finalizer("mpc_recurrent_policy_destroy")

    def state(self, n):
        """(h, c) for ``n`` robots; a new ``n`` starts from zero state."""
        import torch
        if self.h is None or self.h.shape[0] != n:
            self.h = torch.zeros((n, self.hidden_size), dtype=torch.float32, device=self.device)
            self.c = torch.zeros_like(self.h)
        return self.h, self.c

    def reset_memory(self, env_ids=None):
        """Zero state for every robot, or for the robots ``env_ids`` (a device index tensor, or anything ``torch.as_tensor`` takes); nothing is
        read back to the host."""
        import torch
        if self.h is None:
            return
        if env_ids is None:
            self.h.zero_(); self.c.zero_()
            return
        ids = torch.as_tensor(env_ids, dtype=torch.long, device=self.device)
        self.h.index_fill_(0, ids, 0.0); self.c.index_fill_(0, ids, 0.0)

    def step(self, obs, reset=None, return_actions=False):
        """obs [n, I] -> MPC weights [n, 12] (and the raw actor output if asked); the memory advances.  ``reset`` [n] int64 or None: where
        non-zero the robot's memory is taken as zero before the step (the task's reset tensor of the tick before)."""
        import torch
        n = obs.shape[0]
        _lib.tensor_arg(obs, torch.float32, n * self.num_obs, "obs")
        if reset is not None:
            _lib.tensor_arg(reset, torch.long, n, "reset")
        h, c = self.state(n)
        weights = torch.empty((n, self.num_actions), dtype=torch.float32, device=self.device)
        actions = torch.empty_like(weights) if return_actions else None
        recurrent_check(recurrent_lib().mpc_recurrent_policy_step(self._handle, n, obs.data_ptr(), h.data_ptr(), c.data_ptr(),
                                                                  reset.data_ptr() if reset is not None else None, actions.data_ptr() if return_actions else None,
                                                                  weights.data_ptr(), _lib.stream(self.device)), "mpc_recurrent_policy_step")
        return (weights, actions) if return_actions else weights
