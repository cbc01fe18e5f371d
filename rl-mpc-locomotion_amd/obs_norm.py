"""Running observation normalisation on the device (include/mpc_obs_norm.h, csrc/mpc_obs_norm.hip, csrc/obs_norm.h).

rsl_rl 2.x's ``EmpiricalNormalization`` (rl_games' ``normalize_input``): per column of the [n, D] float32 observations a running mean and
population variance over every row seen so far, and ``y = (x - mean) / (std + eps)``:

    norm = ObsNormalizer(env.num_obs)                    # eps = 1e-2, rsl_rl's default
    obs = norm(env.reset())                              # update, then normalise: three launches, nothing goes to the host
    obs = norm(raw, out=storage.observations[t])         # straight into a slot of the rollout storage (or ``out=raw``: in place)
    action = policy(norm(raw, update=False))             # deployment: one launch

The running state is float64 on the device (``state64`` [2, D]: the means, then the variances; ``count`` int64 rows); the float32 buffers ``_mean``,
``_var``, ``_std`` [1, D] are its roundings, rewritten by every update, and normalisation is float32 on them -- bit for bit numpy's
``(x - _mean) / (_std + eps)``.  A fresh normaliser is rsl_rl's: count 0, mean 0, var 1.  ``until``: an update that finds ``count >= until`` is skipped, decided
on the device.  A row with any non-finite entry is left out of the update and is not counted (rsl_rl would carry the NaN in its statistics for good); it
passes through normalisation as arithmetic leaves it.

``fold_normalizer`` folds a trained normaliser into the first layers of a ``model_state_dict`` for loaders that take raw observations.

The entry points need the GPU (MpcLibraryError without one) and have no CPU fallback.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ci, ll, need_gpu, pvp, text, vp

# the entry points of include/mpc_obs_norm.h (bound here, not in any other module's list)
DECLS = {
    "mpc_obsnorm_create": (ci, [pvp, ci, C.c_float, ll]),
    "mpc_obsnorm_destroy": (None, [vp]),
    "mpc_obsnorm_bind": (ci, [vp, vp]),
    "mpc_obsnorm_apply": (ci, [vp, vp, vp, ll, ci, vp]),
    "mpc_obsnorm_clear": (ci, [vp, vp]),
    "mpc_obsnorm_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS)             # libmpc_batch.so with the normaliser's entry points bound
check = _lib.checker(lib, "mpc_obsnorm_last_error")

MAX_OBS, BLOCK_ROWS = 256, 32


class _Buffers(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("state", "count", "mean", "var", "std")]


class ObsNormalizer:
    """rsl_rl's ``EmpiricalNormalization`` for [n, num_obs] float32 cuda observations, 1 <= num_obs <= 256, any n >= 1 per call.

    Public device tensors: ``_mean``, ``_var``, ``_std`` [1, num_obs] float32, ``count`` int64 (a scalar tensor, as rsl_rl's), ``state64``
    [2, num_obs] float64.  ``guard`` (for tests) puts that many spare elements on either side of every one of them."""

    def __init__(self, num_obs, eps=1e-2, until=None, device=None, guard=0):
        need_gpu("ObsNormalizer")
        self.num_obs, self.eps, self.until = int(num_obs), float(eps), None if until is None else int(until)
        if self.until is not None and self.until < 0:
            raise ValueError("until must be None or a row count >= 0")
        self.device = _lib.device_of(device)
        self._handle = C.c_void_p()
        check(lib().mpc_obsnorm_create(C.byref(self._handle), self.num_obs, self.eps, -1 if self.until is None else self.until), "mpc_obsnorm_create")
        D, g = self.num_obs, int(guard)
        self._raw = {}

        def z(name, shape, dtype):
            numel = 1
            for k in shape:
                numel *= k
            self._raw[name] = torch.zeros(numel + 2 * g, dtype=dtype, device=self.device)
            return self._raw[name][g:g + numel].view(shape)
        self.state64, self.count = z("state64", (2, D), torch.float64), z("count", (), torch.long)
        self._mean, self._var, self._std = z("_mean", (1, D), torch.float32), z("_var", (1, D), torch.float32), z("_std", (1, D), torch.float32)
        b = _Buffers(*(t.data_ptr() for t in (self.state64, self.count, self._mean, self._var, self._std)))
        with torch.cuda.device(self.device):
            check(lib().mpc_obsnorm_bind(self._handle, C.addressof(b)), "mpc_obsnorm_bind")
        self.clear()

    __del__ = _lib.finalizer("mpc_obsnorm_destroy")

    def __call__(self, obs, out=None, update=True):
        """``update``: the batch is first merged into the running state (rsl_rl's ``forward`` in training: update, then normalise), so the
        statistics include the rows they normalise.  ``out``: ``obs`` itself (in place) or any other contiguous [n, num_obs] float32 cuda tensor
        that does not otherwise overlap ``obs``; a fresh tensor when None.  Stream-ordered, no host synchronisation -- except that the first batch with
        more rows than any before it allocates the workspace of partials."""
        need_gpu("ObsNormalizer", obs)
        if obs.dtype != torch.float32 or obs.dim() != 2 or obs.shape[1] != self.num_obs or obs.shape[0] < 1 or not obs.is_contiguous() or obs.device != self.device:
            raise ValueError(f"obs must be a contiguous float32 [n >= 1, {self.num_obs}] tensor on {self.device}")
        if out is None:
            out = torch.empty_like(obs)
        elif out.dtype != torch.float32 or out.shape != obs.shape or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 {tuple(obs.shape)} tensor on {self.device}")
        check(lib().mpc_obsnorm_apply(self._handle, obs.data_ptr(), out.data_ptr(), obs.shape[0], 1 if update else 0, _lib.stream(self.device)),
              "mpc_obsnorm_apply")
        return out

    def clear(self):
        """Back to the fresh state: count 0, mean 0, var 1 (and the float32 buffers with them)."""
        check(lib().mpc_obsnorm_clear(self._handle, _lib.stream(self.device)), "mpc_obsnorm_clear")

    def state_dict(self):
        """rsl_rl's four keys (``_mean``, ``_var``, ``_std`` float32 [1, D], ``count`` int64) and ``state64`` (float64 [2, D]: with it a resumed run
        continues bit for bit).  Copies, on the device."""
        return {"_mean": self._mean.clone(), "_var": self._var.clone(), "_std": self._std.clone(), "count": self.count.clone(), "state64": self.state64.clone()}

    def load_state_dict(self, sd):
        """Accepts a dict without ``state64`` (rsl_rl's own): the float64 state is then the widened float32 values."""
        D = self.num_obs
        for k in ("_mean", "_var", "_std"):
            if tuple(sd[k].shape) != (1, D):
                raise ValueError(f"{k} must have shape (1, {D})")
        s64 = sd.get("state64")
        if s64 is not None and tuple(s64.shape) != (2, D):
            raise ValueError(f"state64 must have shape (2, {D})")
        for k, t in (("_mean", self._mean), ("_var", self._var), ("_std", self._std)):
            t.copy_(sd[k].to(torch.float32))
        self.count.copy_(torch.as_tensor(sd["count"]).to(torch.long).reshape(()))
        if s64 is not None:
            self.state64.copy_(s64.to(torch.float64))
        else:
            self.state64[0].copy_(sd["_mean"][0].to(torch.float64))
            self.state64[1].copy_(sd["_var"][0].to(torch.float64))


def fold_normalizer(model_state_dict, obs_norm_state_dict, eps=1e-2, critic_obs_norm_state_dict=None):
    """A ``model_state_dict`` whose actor and critic take RAW observations: the normaliser folded into layer 0,
    ``W'[:, c] = W[:, c] / (std_c + eps)`` and ``b' = b - W' mean``, computed in float64 from the float32 buffers (``std_c + eps`` as the float32 sum
    normalisation uses) and rounded once; every other key passes through untouched.  ``eps`` is the normaliser's.  ``WeightPolicy.from_state_dict``
    and the reference's loader then run a policy trained with normalisation unchanged.  ``critic_obs_norm_state_dict``: the statistics of the critic's
    own rows (a checkpoint of an asymmetric run carries them), folded into the critic in place of the actor's.

    A recurrent ``model_state_dict`` (``memory_a.rnn.weight_ih_l0``): the observations enter through the memories, so the same formula folds the
    actor's statistics into ``memory_a.rnn.weight_ih_l0`` / ``bias_ih_l0`` and the critic's (the actor's when there are none) into ``memory_c.rnn``'s;
    ``actor.0`` / ``critic.0`` read the memories' outputs and pass through.

    The limit: where ``|mean_c| >> std_c`` the folded layer computes ``W' x - W' mean`` in float32 and the two cancel; a caller who needs better
    runs ``ObsNormalizer(...)(obs, update=False)`` in front of ``WeightPolicy.step`` instead."""
    out = dict(model_state_dict)
    recurrent = "memory_a.rnn.weight_ih_l0" in out
    for net, memory in (("actor", "memory_a"), ("critic", "memory_c")):
        wk, bk = (f"{memory}.rnn.weight_ih_l0", f"{memory}.rnn.bias_ih_l0") if recurrent else (f"{net}.0.weight", f"{net}.0.bias")
        if wk not in out:
            continue
        sd = critic_obs_norm_state_dict if net == "critic" and critic_obs_norm_state_dict is not None else obs_norm_state_dict
        mean = sd["_mean"].reshape(-1)
        std = sd["_std"].reshape(-1).to(torch.float32)
        scale = (std + torch.tensor(eps, dtype=torch.float32, device=std.device)).to(torch.float64)
        W, b = out[wk], out[bk]
        if W.shape[1] != mean.numel():
            raise ValueError(f"{wk} takes {W.shape[1]} observations, the normaliser has {mean.numel()}")
        W64 = W.to(torch.float64) / scale.to(W.device)
        out[wk] = W64.to(W.dtype)
        out[bk] = (b.to(torch.float64) - W64 @ mean.to(W.device, torch.float64)).to(b.dtype)
    return out
