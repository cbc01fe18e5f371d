"""A recurrent (LSTM) actor-critic: the device cell step, the trajectories of the update through time and its device form (csrc/mpc_recurrent.h,
csrc/mpc_recurrent.hip, csrc/recurrent_cell.h; csrc/mpc_recurrent_bptt.h, csrc/mpc_recurrent_bptt.hip, csrc/recurrent_bptt.h).

rsl_rl v1.0.2's ``Memory``, ``ActorCriticRecurrent``, ``split_and_pad_trajectories`` / ``unpad_trajectories`` by their published algorithms (rsl_rl
is an empty submodule in the reference): a one-layer LSTM in front of the actor's MLP and another in front of the critic's, so that the actor can
infer from the history of its rows what one row does not show -- the payload, the motor strength and the gravity of ``plant_rand``.  The MLPs read the
memories' outputs: their first layers are ``rnn_hidden_size`` wide (rsl_rl's ``super().__init__(num_actor_obs=rnn_hidden_size, ...)``).

* the **collection half** is HIP: ``ActorCriticRecurrent.act`` is two launches, ``mpc_recurrent_step`` (both memories side by side; the state per
  environment lives on the device, is zeroed inside the step where the task's reset flag of the tick before is set, and the state the step started from is
  written straight into slot t of the storage) and then ``ActorCritic.act`` on the two outputs.  The kernel reads the LSTM's parameters where the
  optimiser updates them in place.
* the **update half** is torch: ``RolloutStorage.recurrent_mini_batch_generator`` cuts every environment's column into trajectories at the episode
  ends and pads them, ``log_prob_entropy_value`` runs ``nn.LSTM`` over them from the saved state and autograd goes back through time.
* ``RecurrentConfig(update_through_time="hip")`` (opt-in; "torch", the default, launches what it always launched) takes the memories' part of that update
  to the device: ``RolloutStorage.recurrent_sequence_generator`` yields the dense ``[T][block]`` roll of each block of environments -- strided views of
  the storage and the reset flags ``reset[t] = dones[t-1]``, no padding, no host read -- and ``log_prob_entropy_value(reset=...)`` runs both memories
  over it in ONE launch (``mpc_recurrent_bptt_forward``) inside ONE ``torch.autograd.Function`` over both memories' parameters, whose backward is
  ``mpc_recurrent_bptt_backward``.  The dense roll equals the padded trajectories because the collection stores zero in ``saved_*[t]`` after a done.
  The MLPs, the loss, the clip and Adam stay torch's; ``PPO(backend="hip")`` still refuses a recurrent actor-critic: the MLPs, the loss head and Adam
  of a recurrent device update are not built.
* ``RecurrentConfig(update_through_time="hip", update_heads="hip")`` (opt-in on top of the former) takes the rest of the update to the device as well:
  per mini-batch the forward roll into two persistent ``[T B][H]`` buffers, ``mpc_ppo_update_grads_sequence`` (the MLPs on those dense rows, the loss
  head on the storage through a row index, the MLPs' backward pass down to the gradient of the rows), the backward pass through time straight into the
  memories' ``.grad``, and ONE clip and Adam step over the MLPs' and the memories' tensors (``mpc_ppo_update_bind_extra``) -- one stream, no host read,
  no autograd (``PPO._update_recurrent_hip``).  The mini-batches are ``recurrent_sequence_generator``'s blocks.

    trainer = PPOTrainer(env, recurrent=RecurrentConfig(hidden_size=256))                                  # update_through_time="hip": see above
    trainer.learn(num_iterations)

Two stated deviations from v1.0.2.  ``evaluate`` does not advance the critic's memory: rsl_rl's stepping-mode ``evaluate`` advances it on the
iteration's last row, and the next ``act`` consumes that row a second time; here ``last_values`` is a peek and every row advances each memory exactly
once.  ``split_and_pad_trajectories`` pads every piece to T, always: v1.0.2 pads to the longest piece, and its ``unpad_trajectories`` then fails when
every environment had a ``done``.

Deployment: ``WeightPolicy.from_state_dict`` on a recurrent checkpoint's ``model_state_dict`` gives a ``weight_policy.RecurrentWeightPolicy``, whose ``step`` is
``memory_a``'s cell and the actor in one launch (csrc/recurrent_policy.h).

Not built: GRU, stacked layers.  ``PPO(backend="hip")`` keeps refusing a recurrent actor-critic: its device update is spelled ``update_heads="hip"``.

The torch paths (``step_torch``, ``log_prob_entropy_value``, ``Memory.forward_sequence`` without the option, the split / pad functions) run on the CPU in
any dtype; the device entry points need the GPU (MpcLibraryError without one) and have no CPU fallback.
"""
import ctypes as C
from collections import namedtuple
from dataclasses import dataclass

import torch
from torch import nn

from . import _lib
from ._lib import ci, ll, need_gpu, pvp, tensor_arg, text, vp
from .ppo import NUM_ACTIONS, ActorCritic

MEMORIES = 2                           # csrc/mpc_recurrent.h's MPC_RECURRENT_MEMORIES: the actor's, the critic's
ACTOR, CRITIC = 0, 1


class Io(C.Structure):
    """csrc/mpc_recurrent.h's ``mpc_recurrent_io``."""
    _fields_ = [(k, vp) for k in ("d_x", "d_h", "d_c", "d_h_saved", "d_c_saved", "d_h_out")]


# the entry points of csrc/mpc_recurrent.h (bound here, not in any other module's list)
DECLS = {
    "mpc_recurrent_create": (ci, [pvp, ci, vp, vp]),
    "mpc_recurrent_destroy": (None, [vp]),
    "mpc_recurrent_bind": (ci, [vp, vp, vp, vp, vp]),
    "mpc_recurrent_step": (ci, [vp, ci, ci, ci, vp, vp, ci, vp]),
    "mpc_recurrent_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS)
check = _lib.checker(lib, "mpc_recurrent_last_error")


class SeqIo(C.Structure):
    """csrc/mpc_recurrent_bptt.h's ``mpc_recurrent_bptt_io``."""
    _fields_ = [("d_x", vp), ("x_stride", ll), ("d_h0", vp), ("d_c0", vp), ("d_y", vp), ("d_c_last", vp)]


class SeqGrads(C.Structure):
    """csrc/mpc_recurrent_bptt.h's ``mpc_recurrent_bptt_grads``."""
    _fields_ = [(k, vp) for k in ("d_dy", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh")]


# the entry points of csrc/mpc_recurrent_bptt.h
BPTT_DECLS = {
    "mpc_recurrent_bptt_create": (ci, [pvp, ci, vp, vp, ci, ci]),
    "mpc_recurrent_bptt_destroy": (None, [vp]),
    "mpc_recurrent_bptt_workspace_bytes": (ll, [vp]),
    "mpc_recurrent_bptt_bind": (ci, [vp, vp, vp, vp, vp]),
    "mpc_recurrent_bptt_forward": (ci, [vp, ci, ci, ci, ci, vp, vp, vp]),
    "mpc_recurrent_bptt_backward": (ci, [vp, ci, ci, ci, ci, vp, vp]),
    "mpc_recurrent_bptt_weight_gradients": (ci, [vp, ci, ci, ci, ci, vp, vp]),
    "mpc_recurrent_bptt_dgates": (ci, [vp, ci, pvp]),
    "mpc_recurrent_bptt_last_error": (text, []),
}
BPTT_SYMBOLS = list(BPTT_DECLS)
bptt_lib = _lib.binder(BPTT_DECLS)
bptt_check = _lib.checker(bptt_lib, "mpc_recurrent_bptt_last_error")

THROUGH_TIME = ("torch", "hip")


def through_time_option(value):
    if value not in THROUGH_TIME:
        raise ValueError(f"update_through_time={value!r}: 'torch' or 'hip'")
    return value


def heads_option(value, through_time):
    """``update_heads`` beside ``update_through_time``: the device heads read the device roll's buffers, so "hip" needs "hip" there."""
    if value not in THROUGH_TIME:
        raise ValueError(f"update_heads={value!r}: 'torch' or 'hip'")
    if value == "hip" and through_time != "hip":
        raise ValueError('update_heads="hip" requires update_through_time="hip": the MLPs, the loss head and Adam on the device read the device roll\'s '
                         'outputs and feed its backward pass')
    return value


@dataclass
class RecurrentConfig:
    """rsl_rl's ``rnn_type``, ``rnn_hidden_size`` and ``rnn_num_layers``; one LSTM layer is what is built.  ``update_through_time``: "torch" (the
    default: ``nn.LSTM`` over padded trajectories, autograd back through time) or "hip" (the dense roll and its backward pass on the device).
    ``update_heads``: "torch" (the default: torch's MLPs, loss, clip and Adam) or "hip" (those on the device too; needs ``update_through_time="hip"``)."""
    hidden_size: int = 256
    rnn_type: str = "lstm"
    num_layers: int = 1
    update_through_time: str = "torch"
    update_heads: str = "torch"

    def __post_init__(self):
        through_time_option(self.update_through_time)
        heads_option(self.update_heads, self.update_through_time)


# what ``RolloutStorage.recurrent_mini_batch_generator`` yields: padded trajectories and masks, [T][block] slices, each memory's (h0, c0)
RecurrentBatch = namedtuple("RecurrentBatch", "obs critic_obs masks actions values advantages returns old_log_prob old_mu old_sigma hidden_a hidden_c")
# what ``RolloutStorage.recurrent_sequence_generator`` yields: the dense roll of a block of environments -- views [T][block][width] of the storage, the
# flags reset [T][block] int64 (reset[0] = 0, reset[t] = dones[t-1]), the same [T][block] slices, each memory's (h0, c0) [block][H] = saved_*[0]
RecurrentSequenceBatch = namedtuple("RecurrentSequenceBatch",
                                    "obs critic_obs reset actions values advantages returns old_log_prob old_mu old_sigma hidden_a hidden_c")


def refuse_unbuilt(rnn_type, rnn_num_layers):
    if str(rnn_type).lower() != "lstm":
        raise ValueError(f"rnn_type={rnn_type!r}: not built (LSTM only)")
    if int(rnn_num_layers) != 1:
        raise ValueError(f"rnn_num_layers={rnn_num_layers}: not built (one layer only)")


# ---- trajectories ---------------------------------------------------------------------------------------------------------------------------------
def trajectory_masks(dones):
    """dones [T][N][1] -> (masks [T][n_traj] bool, starts [N][T] bool): every environment's column is cut after each done (and after its last
    slot); trajectory k, counted environment-major, is ``masks[:, k].sum()`` steps long, and ``starts[e][t]`` is set where a trajectory of
    environment e begins (t = 0, or the step after a done).  One host read (the number of trajectories)."""
    T = dones.shape[0]
    d = dones.clone()
    d[-1] = 1
    flat = d.transpose(1, 0).reshape(-1) != 0                                  # environment-major
    ends = flat.nonzero()[:, 0]
    lengths = ends - torch.cat((ends.new_full((1,), -1), ends[:-1]))
    masks = lengths.unsqueeze(0) > torch.arange(T, device=dones.device).unsqueeze(1)
    starts = torch.ones_like(flat).view(-1, T)
    starts[:, 1:] = flat.view(-1, T)[:, :-1]
    return masks, starts


def split_and_pad_trajectories(tensor, dones):
    """rsl_rl's: tensor [T][N][F], dones [T][N][1] -> (padded [T][n_traj][F], masks [T][n_traj] bool).  The pieces of every environment's column
    between its dones, in environment-major order, each padded with zeros to length T -- always T (v1.0.2 pads to the longest piece)."""
    masks, _ = trajectory_masks(dones)
    return pad_trajectories(tensor, masks), masks


def pad_trajectories(tensor, masks):
    """tensor [T][N][F] cut and padded by the ``masks`` of its dones (``trajectory_masks``) -> [T][n_traj][F]."""
    padded = tensor.new_zeros((tensor.shape[0], masks.shape[1]) + tuple(tensor.shape[2:]))
    padded.transpose(1, 0)[masks.transpose(1, 0)] = tensor.transpose(1, 0).flatten(0, 1)      # consecutive pieces of the environment-major order
    return padded


def unpad_trajectories(x, masks):
    """The inverse of ``split_and_pad_trajectories``: x [T][n_traj][F] -> [T][envs][F]."""
    T = x.shape[0]
    return x.transpose(1, 0)[masks.transpose(1, 0)].view(-1, T, x.shape[-1]).transpose(1, 0)


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """One LSTM step written out (torch's gate order i, f, g, o), in the dtype of its arguments."""
    gates = nn.functional.linear(x, w_ih, b_ih) + nn.functional.linear(h, w_hh, b_hh)
    i, f, g, o = gates.chunk(4, dim=-1)
    c1 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c1), c1


def _memory_sizes(memories):
    """create's two size arrays: the memories' input and hidden sizes."""
    return _lib.int_array([m.input_size for m in memories]), _lib.int_array([m.hidden_size for m in memories])


class SequenceKernel:
    """A handle of csrc/mpc_recurrent_bptt.h over ``memories`` (one ``Memory``, or the actor's and the critic's): the roll over T slots and its
    backward pass.  The handle is made for the first call's (T, B) and made anew for a larger one; the parameters are bound by pointer and bound
    again when a tensor has moved.  The workspace holds ONE forward call: ``token`` counts them, and a backward call names the forward it belongs to."""

    def __init__(self, memories):
        self.memories = tuple(memories)
        self._handle, self._ptrs, self.max_steps, self.max_rows, self.token = None, None, 0, 0, 0

    __del__ = _lib.finalizer("mpc_recurrent_bptt_destroy")

    def workspace_bytes(self):
        return 0 if self._handle is None else int(bptt_lib().mpc_recurrent_bptt_workspace_bytes(self._handle))

    def _ready(self, T, B, device):
        n = len(self.memories)
        if self._handle is None or T > self.max_steps or B > self.max_rows:
            if self._handle is not None:
                bptt_lib().mpc_recurrent_bptt_destroy(self._handle)
                self._handle, self._ptrs = None, None
            h = C.c_void_p()
            steps, rows = max(T, self.max_steps), max(B, self.max_rows)
            bptt_check(bptt_lib().mpc_recurrent_bptt_create(C.byref(h), n, *_memory_sizes(self.memories), steps, rows), "mpc_recurrent_bptt_create")
            self._handle, self.max_steps, self.max_rows = h, steps, rows
        params = [p for m in self.memories for p in m.parameters_in_bind_order()]      # (bind's k-th array is every fourth address from k)
        ptrs = _lib.addresses_to_bind(params, self._ptrs, device, "the memories' parameters must be contiguous float32 tensors on the rows' device")
        if ptrs is not None:
            with torch.cuda.device(device):
                bptt_check(bptt_lib().mpc_recurrent_bptt_bind(self._handle, *(_lib.ptr_array(ptrs[k::4]) for k in range(4))), "mpc_recurrent_bptt_bind")
            self._ptrs = ptrs

    def forward(self, which, xs, h0s, c0s, reset, c_last=False, what="SequenceKernel.forward", out=None):
        """ONE launch: the memories ``which`` (consecutive) over xs[k] [T][B][I_k] (a view whose rows are I_k apart and whose slots are a
        multiple of 4 floats apart), from (h0s[k], c0s[k]) [B][H_k]; reset [T][B] int64 or None.  -> [y_k [T][B][H_k]] (and [c' of the last step]).
        ``out`` (for tests): per memory the tensors (y, c_last or None) to write instead of new ones."""
        need_gpu(what, *xs, *h0s, *c0s)
        T, B, dev = xs[0].shape[0], xs[0].shape[1], xs[0].device
        self._ready(T, B, dev)
        if reset is not None:
            need_gpu(what, reset)
            tensor_arg(reset, torch.long, T * B, "reset")
        io, ys, cl = (SeqIo * len(which))(), [], []
        for k, w in enumerate(which):
            m, x = self.memories[w], xs[k]
            if x.dtype != torch.float32 or tuple(x.shape) != (T, B, m.input_size) or x.stride(2) != 1 or x.stride(1) != m.input_size:
                raise ValueError(f"memory {w}: x must be a float32 [T={T}][B={B}][{m.input_size}] tensor or view with contiguous rows")
            tensor_arg(h0s[k], torch.float32, B * m.hidden_size, "h0")
            tensor_arg(c0s[k], torch.float32, B * m.hidden_size, "c0")
            if out is not None:
                y, c1 = out[k]
                tensor_arg(y, torch.float32, T * B * m.hidden_size, "y")
                if c_last:
                    tensor_arg(c1, torch.float32, B * m.hidden_size, "c_last")
            else:
                y = torch.empty((T, B, m.hidden_size), dtype=torch.float32, device=dev)
                c1 = torch.empty((B, m.hidden_size), dtype=torch.float32, device=dev) if c_last else None
            io[k] = SeqIo(x.data_ptr(), x.stride(0) if T > 1 else B * m.input_size, h0s[k].data_ptr(), c0s[k].data_ptr(), y.data_ptr(),
                          c1.data_ptr() if c_last else None)
            ys.append(y); cl.append(c1)
        bptt_check(bptt_lib().mpc_recurrent_bptt_forward(self._handle, T, B, which[0], len(which), C.cast(io, C.c_void_p),
                                                         reset.data_ptr() if reset is not None else None, _lib.stream(dev)), "mpc_recurrent_bptt_forward")
        self.token += 1
        return (ys, cl) if c_last else ys

    def dgates(self, w, T, B):
        """dG [T][B][4H] of memory ``w`` as the last backward call over (T, B) left it: a view of the handle's workspace."""
        p = C.c_void_p()
        bptt_check(bptt_lib().mpc_recurrent_bptt_dgates(self._handle, w, C.byref(p)), "mpc_recurrent_bptt_dgates")
        return _lib.device_view(p.value, (T, B, 4 * self.memories[w].hidden_size), "<f4", self.memories[w].rnn.weight_hh_l0.device)

    def backward(self, which, T, B, dys, token=None, out=None, entry="mpc_recurrent_bptt_backward"):
        """The backward pass of the last forward call (``token``: that call's, checked) -> per memory (dW_ih, dW_hh, db_ih, db_hh), new tensors
        (or ``out``'s, for tests).  ``entry="mpc_recurrent_bptt_weight_gradients"``: the GEMMs and the reduction alone, on the dG that is there."""
        if token is not None and token != self.token:
            raise RuntimeError("the workspace holds a later forward call: go back through a roll before the next one is run on the same memories")
        dev = dys[0].device
        gr, grads = (SeqGrads * len(which))(), []
        for k, w in enumerate(which):
            m = self.memories[w]
            tensor_arg(dys[k], torch.float32, T * B * m.hidden_size, "dy")
            g = tuple(torch.empty_like(p) for p in m.parameters_in_bind_order()) if out is None else tuple(out[k])
            for t, p in zip(g, m.parameters_in_bind_order()):
                tensor_arg(t, torch.float32, p.numel(), "a gradient output")
            gr[k] = SeqGrads(dys[k].data_ptr(), *(t.data_ptr() for t in g))
            grads.append(g)
        bptt_check(getattr(bptt_lib(), entry)(self._handle, T, B, which[0], len(which), C.cast(gr, C.c_void_p), _lib.stream(dev)), entry)
        return grads


class _SequenceFunction(torch.autograd.Function):
    """The roll of ``len(which)`` memories as ONE autograd node: forward(kernel, which, reset, x.., h0.., c0.., the memories' parameters in bind
    order) -> y per memory.  One node over both memories is how two outputs share one forward launch and one backward call; its backward returns
    the parameter gradients and None for x, h0, c0 and reset (data).  The backward pass reads x again, in place, through the pointer the forward
    call was given: the node keeps the x tensors alive (``save_for_backward``, so an in-place write to one in between is autograd's usual error)
    and refuses rows that have moved."""

    @staticmethod
    def forward(ctx, kernel, which, reset, *tensors):
        n = len(which)
        xs, h0s, c0s = tensors[:n], tensors[n:2 * n], tensors[2 * n:3 * n]
        ys = kernel.forward(which, xs, h0s, c0s, reset, what='update_through_time="hip"')
        ctx.kernel, ctx.which, ctx.token, ctx.shape = kernel, which, kernel.token, (xs[0].shape[0], xs[0].shape[1])
        ctx.x_ptrs = tuple(x.data_ptr() for x in xs)
        ctx.save_for_backward(*xs)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *grad_outputs):
        T, B = ctx.shape
        if tuple(x.data_ptr() for x in ctx.saved_tensors) != ctx.x_ptrs:
            raise RuntimeError("the rows of the forward call have moved: the backward pass reads them in place")
        dys = []
        for w, g in zip(ctx.which, grad_outputs):
            m = ctx.kernel.memories[w]
            dys.append(g.contiguous() if g is not None else torch.zeros((T, B, m.hidden_size), dtype=torch.float32, device=m.rnn.weight_hh_l0.device))
        grads = ctx.kernel.backward(ctx.which, T, B, dys, ctx.token)
        return (None, None, None) + (None,) * (3 * len(ctx.which)) + tuple(t for g in grads for t in g)


def roll_on_device(kernel, which, xs, h0s, c0s, reset):
    """``_SequenceFunction`` over the memories ``which`` of ``kernel`` -> the tuple of their outputs [T][B][H]."""
    params = [p for w in which for p in kernel.memories[w].parameters_in_bind_order()]
    return _SequenceFunction.apply(kernel, tuple(which), reset, *xs, *h0s, *c0s, *params)


class Memory(nn.Module):
    """rsl_rl's ``Memory`` with an LSTM: ``rnn = nn.LSTM(input_size, hidden_size, 1)``, so the state dict has rsl_rl's keys
    (``rnn.weight_ih_l0``, ``weight_hh_l0``, ``bias_ih_l0``, ``bias_hh_l0``).  ``h``, ``c`` [n][H]: the device state, allocated (zero) on first use,
    advanced by ``mpc_recurrent_step``; ``out`` [n][H]: the step's h', what the MLP behind the memory reads.  ``update_through_time``: what
    ``forward_sequence`` runs."""

    def __init__(self, input_size, hidden_size=256, rnn_type="lstm", num_layers=1, update_through_time="torch"):
        super().__init__()
        refuse_unbuilt(rnn_type, num_layers)
        self.update_through_time = through_time_option(update_through_time)
        self.input_size, self.hidden_size = int(input_size), int(hidden_size)
        self.rnn = nn.LSTM(self.input_size, self.hidden_size, 1)
        self.h, self.c, self.out = None, None, None
        self._seq = None

    def parameters_in_bind_order(self):
        return [self.rnn.weight_ih_l0, self.rnn.weight_hh_l0, self.rnn.bias_ih_l0, self.rnn.bias_hh_l0]

    def state(self, n, device):
        """(h, c, out) for ``n`` rows on ``device``; a new size or device starts from zero state."""
        if self.h is None or self.h.shape[0] != n or self.h.device != device:
            z = lambda: torch.zeros((n, self.hidden_size), dtype=torch.float32, device=device)
            self.h, self.c, self.out = z(), z(), z()
        return self.h, self.c, self.out

    def reset(self):
        if self.h is not None:
            self.h.zero_()
            self.c.zero_()

    def step_torch(self, x, state=None, reset=None):
        """One tick in torch: x [n][I], state (h, c) or None (zero), reset [n] or None -> (h', (h', c'), the state the step started from)."""
        n = x.shape[0]
        h, c = state if state is not None else (x.new_zeros((n, self.hidden_size)), x.new_zeros((n, self.hidden_size)))
        if reset is not None:
            keep = (reset.reshape(n, 1) == 0).to(x.dtype)
            h, c = h * keep, c * keep
        h1, c1 = lstm_cell(x, h, c, *self.parameters_in_bind_order())
        return h1, (h1, c1), (h, c)

    def forward_sequence(self, x, h0, c0, reset=None):
        """The dense roll: x [T][B][I] from (h0, c0) [B][H]; where reset[t][b] (``[T][B]``, or None) is set the state of row b is zero before step
        t -> h' [T][B][H].  Without the option: a differentiable loop of ``lstm_cell`` on any device in any dtype.  With ``update_through_time="hip"``:
        one launch on GPU tensors (MpcLibraryError for others) inside a ``torch.autograd.Function`` whose backward is the device's; x, h0, c0 get no
        gradient."""
        if self.update_through_time == "hip":
            need_gpu('Memory.forward_sequence with update_through_time="hip"', x, h0, c0)
            if self._seq is None:
                self._seq = SequenceKernel((self,))
            return roll_on_device(self._seq, (0,), (x,), (h0,), (c0,), reset)[0]
        h, c, out = h0, c0, []
        for t in range(x.shape[0]):
            if reset is not None:
                keep = (reset[t] == 0).to(x.dtype).unsqueeze(-1)
                h, c = h * keep, c * keep
            h, c = lstm_cell(x[t], h, c, *self.parameters_in_bind_order())
            out.append(h)
        return torch.stack(out)

    def forward(self, padded, masks, hidden):
        """Batch mode: padded [T][n_traj][I] from ``hidden`` = (h0, c0) [1][n_traj][H] -> [T][envs][H]."""
        out, _ = self.rnn(padded, hidden)
        return unpad_trajectories(out, masks) if masks is not None else out


class ActorCriticRecurrent(ActorCritic):
    """rsl_rl's ``ActorCriticRecurrent``: ``memory_a`` reads the actor's rows (``num_obs`` wide), ``memory_c`` the critic's (``num_critic_obs`` wide
    if given, ``num_obs`` otherwise), and the parent's MLPs read the memories' outputs (``rnn_hidden_size`` wide each).  The state dict has rsl_rl's
    keys: the parent's and ``memory_{a,c}.rnn.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0}``.

    ``act`` is the cell launch and then the parent's asymmetric ``act``.  ``reset``: the task's reset tensor (int64 [n]) of the tick before, or None;
    where it is set the row's state is taken as zero before the step.  ``saved``: dict of ``h_a``, ``c_a``, ``h_c``, ``c_c`` [n][H] views
    (``RolloutStorage.hidden_slot(t)``) that receive the state the step started from.  ``evaluate`` peeks: it does not advance the critic's memory.
    ``update_through_time`` / ``update_heads``: ``RecurrentConfig``'s."""
    is_recurrent = True

    def __init__(self, num_obs=48, num_actions=NUM_ACTIONS, actor_hidden_dims=(512, 256, 128), critic_hidden_dims=(512, 256, 128), init_noise_std=1.0,
                 num_critic_obs=None, rnn_type="lstm", rnn_hidden_size=256, rnn_num_layers=1, update_through_time="torch", update_heads="torch"):
        refuse_unbuilt(rnn_type, rnn_num_layers)
        through_time_option(update_through_time)
        heads_option(update_heads, update_through_time)
        H = int(rnn_hidden_size)
        super().__init__(H, num_actions, actor_hidden_dims, critic_hidden_dims, init_noise_std, num_critic_obs=H)
        self.obs_width = int(num_obs)                                            # what memory_a reads
        self.critic_obs_width = int(num_obs if num_critic_obs is None else num_critic_obs)
        self.privileged = num_critic_obs is not None                             # the critic's memory reads rows of its own
        self.rnn_hidden_size = H
        self.hidden_sizes = (H, H)                                               # what a RolloutStorage keeps per slot: (h, c) of memory_a, of memory_c
        self.memory_a = Memory(self.obs_width, H)
        self.memory_c = Memory(self.critic_obs_width, H)
        self._cell_handle, self._cell_ptrs = None, None
        self.update_through_time = update_through_time
        self.update_heads = update_heads                                         # "hip": PPO.update runs the whole update on the device
        self._seq = None                                                         # the update through time's handle over both memories (first use)

    _destroy_cell = _lib.finalizer("mpc_recurrent_destroy", attr="_cell_handle")
    _destroy_ac = ActorCritic.__del__

    def __del__(self):                                                           # (through the class: at interpreter exit this module's globals are gone)
        self._destroy_cell()
        self._destroy_ac()

    def memories(self):
        return (self.memory_a, self.memory_c)

    def reset_memory(self):
        """rsl_rl's ``reset()`` for every environment: all state to zero."""
        for m in self.memories():
            m.reset()

    # ---- the device path -----------------------------------------------------------------------------------------------------------------------
    def _cell_ready(self, what, device):
        need_gpu(what, self.std)
        if self._cell_handle is None:
            h = C.c_void_p()
            check(lib().mpc_recurrent_create(C.byref(h), MEMORIES, *_memory_sizes(self.memories())), "mpc_recurrent_create")
            self._cell_handle = h
        params = [p for m in self.memories() for p in m.parameters_in_bind_order()]
        ptrs = _lib.addresses_to_bind(params, self._cell_ptrs, device, "the memories' parameters must be contiguous float32 tensors on the observations' device")
        if ptrs is not None:
            with torch.cuda.device(device):
                check(lib().mpc_recurrent_bind(self._cell_handle, *(_lib.ptr_array(ptrs[k::4]) for k in range(4))), "mpc_recurrent_bind")
            self._cell_ptrs = ptrs

    def cell_step(self, rows, reset=None, saved=None, commit=True, what="ActorCriticRecurrent.cell_step"):
        """ONE launch of ``mpc_recurrent_step``.  ``rows``: ``{ACTOR: obs}``, ``{CRITIC: critic rows}`` or both (consecutive memories); returns
        the stepped memories' ``out`` tensors in that order."""
        which = sorted(rows)
        x0 = rows[which[0]]
        need_gpu(what, *rows.values())
        n, dev = x0.shape[0], x0.device
        self._cell_ready(what, dev)
        if reset is not None:
            need_gpu(what, reset)
            tensor_arg(reset, torch.long, n, "reset")
        io, outs = (Io * len(which))(), []
        for k, w in enumerate(which):
            m = self.memories()[w]
            tensor_arg(rows[w], torch.float32, n * m.input_size, "critic_obs" if w == CRITIC else "obs")
            h, c, out = m.state(n, dev)
            sv = (None, None)
            if saved is not None:
                sv = (saved["h_c"], saved["c_c"]) if w == CRITIC else (saved["h_a"], saved["c_a"])
                for t in sv:
                    tensor_arg(t, torch.float32, n * m.hidden_size, "saved")
            io[k] = Io(rows[w].data_ptr(), h.data_ptr(), c.data_ptr(), *(t.data_ptr() if t is not None else None for t in sv), out.data_ptr())
            outs.append(out)
        check(lib().mpc_recurrent_step(self._cell_handle, n, which[0], len(which), C.cast(io, C.c_void_p), reset.data_ptr() if reset is not None else None,
                                       int(bool(commit)), _lib.stream(dev)), "mpc_recurrent_step")
        return outs

    def _critic_rows(self, obs, critic_obs):
        if critic_obs is None and self.privileged:
            raise ValueError("this actor-critic was made with num_critic_obs: the critic's memory needs critic_obs")
        return obs if critic_obs is None else critic_obs

    def act(self, obs, seed, step, out=None, return_eps=False, critic_obs=None, reset=None, saved=None):
        """Two launches: both memories advance on (obs, critic rows), then ``ActorCritic.act`` on (h_a', h_c') -- the same dict as the parent's."""
        h_a, h_c = self.cell_step({ACTOR: obs, CRITIC: self._critic_rows(obs, critic_obs)}, reset, saved, True, "ActorCriticRecurrent.act")
        return super().act(h_a, seed, step, out=out, return_eps=return_eps, critic_obs=h_c)

    def evaluate(self, critic_obs, out=None, reset=None):
        """The critic's value of rows [n, critic_obs_width] from the critic's memory as it stands (``reset`` applied), WITHOUT advancing it."""
        h_c, = self.cell_step({CRITIC: critic_obs}, reset, None, False, "ActorCriticRecurrent.evaluate")
        return super().evaluate(h_c, out=out)

    def act_inference(self, obs, reset=None):
        """The actor's mean; steps ``memory_a`` only."""
        h_a, = self.cell_step({ACTOR: obs}, reset, None, True, "ActorCriticRecurrent.act_inference")
        return super().act_inference(h_a)

    # ---- the torch paths (differentiable, any device, any dtype) ------------------------------------------------------------------------------------
    def step_torch(self, obs, critic_obs=None, state=None, reset=None):
        """One tick: ``state`` = ((h_a, c_a), (h_c, c_c)) or None (zero) -> (mu [n,12], value [n,1], the new state, the state the step started
        from after the reset's zeroing -- what the storage keeps for the slot)."""
        sa, sc = state if state is not None else (None, None)
        h_a, new_a, used_a = self.memory_a.step_torch(obs, sa, reset)
        h_c, new_c, used_c = self.memory_c.step_torch(self._critic_rows(obs, critic_obs), sc, reset)
        return self.actor(h_a), self.critic(h_c), (new_a, new_c), (used_a, used_c)

    def forward_sequences(self, obs, critic_rows, hidden_states, reset):
        """Both memories over the dense roll of a block -> (h_a' [T][B][H], h_c' [T][B][H]).  "torch": two ``Memory.forward_sequence`` loops.  "hip":
        ONE forward launch and ONE autograd node over both memories' parameters (``_SequenceFunction``)."""
        (h0_a, c0_a), (h0_c, c0_c) = hidden_states
        if self.update_through_time != "hip":
            return self.memory_a.forward_sequence(obs, h0_a, c0_a, reset), self.memory_c.forward_sequence(critic_rows, h0_c, c0_c, reset)
        need_gpu('ActorCriticRecurrent with update_through_time="hip"', obs, critic_rows, h0_a, c0_a, h0_c, c0_c)
        if self._seq is None:
            self._seq = SequenceKernel(self.memories())
        return roll_on_device(self._seq, (ACTOR, CRITIC), (obs, critic_rows), (h0_a, h0_c), (c0_a, c0_c), reset)

    def log_prob_entropy_value(self, obs, actions, critic_obs=None, masks=None, hidden_states=None, reset=None):
        """Batch mode: ``obs`` (and ``critic_obs``) are padded trajectories [T][n_traj][width], ``hidden_states`` = ((h0_a, c0_a), (h0_c, c0_c)), each
        [1][n_traj][H], their first steps' saved states, ``masks`` [T][n_traj]; ``rnn(padded, (h0, c0))``, then unpad, then the MLPs.  ``actions``
        [T][envs][12] -> (log-prob [T][envs], entropy [T][envs], value [T][envs][1], mu, sigma [T][envs][12]).

        The dense form, when the batch carries ``reset`` [T][block] instead of ``masks``: ``obs`` (and ``critic_obs``) are the block's rows
        [T][block][width] as they lie in the storage, ``hidden_states`` each [block][H], the state slot 0 started from; ``forward_sequences``."""
        if hidden_states is None:
            raise ValueError("batch mode needs the trajectories' first hidden states")
        if reset is not None:
            if masks is not None:
                raise ValueError("a batch carries masks (padded trajectories) or reset (the dense roll), not both")
            h_a, h_c = self.forward_sequences(obs, self._critic_rows(obs, critic_obs), hidden_states, reset)
            mu, value = self.actor(h_a), self.critic(h_c)
            dist = torch.distributions.Normal(mu, mu * 0. + self.std)
            return dist.log_prob(actions).sum(dim=-1), dist.entropy().sum(dim=-1), value, mu, dist.stddev
        mu = self.actor(self.memory_a(obs, masks, hidden_states[0]))
        value = self.critic(self.memory_c(self._critic_rows(obs, critic_obs), masks, hidden_states[1]))
        dist = torch.distributions.Normal(mu, mu * 0. + self.std)
        return dist.log_prob(actions).sum(dim=-1), dist.entropy().sum(dim=-1), value, mu, dist.stddev
