"""ctypes loader of the C-ABI library (include/mpc_batch.h).  There is NO fallback: if the HIP
library is missing or no GPU is usable, every entry point raises -- the product path never routes
through a CPU implementation."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPC_LIB_PATH", os.path.join(_HERE, "csrc", "libmpc_batch.so"))   # override: kernel-variant experiments
_LIB = None

MPC_OK = 0
vp, ci, cd, ll, pvp, text = C.c_void_p, C.c_int, C.c_double, C.c_longlong, C.POINTER(C.c_void_p), C.c_char_p
# the entry points of include/mpc_batch.h: name -> (restype, argtypes).  Every module that calls into the library declares its header's entry
# points in a table like this one, once; its SYMBOLS and its lib() (binder) follow from the table.
DECLS = {
    "mpc_input_len": (ci, [ci]),
    "mpc_supported_horizons": (ci, [vp, ci]),
    "mpc_batch_create": (ci, [pvp, ci, ci, cd, cd, vp, vp]),
    "mpc_batch_destroy": (None, [vp]),
    "mpc_batch_solve": (ci, [vp, vp, vp, vp, vp]),
    "mpc_batch_set_solver": (ci, [vp, ci]),
    "mpc_batch_set_max_iter": (ci, [vp, ci]),
    "mpc_batch_solve_f64": (ci, [vp, vp, vp, vp, vp]),
    "mpc_batch_solve_f16": (ci, [vp, vp, vp, vp, vp]),
    "mpc_batch_reset": (ci, [vp, vp, ci, vp]),
    "mpc_batch_reset_device": (ci, [vp, vp, ci, vp]),
    "mpc_batch_solve_host": (ci, [vp, vp, vp, vp]),
    "mpc_batch_solve_host_f64": (ci, [vp, vp, vp, vp]),
    "mpc_batch_size": (ci, [vp]),
    "mpc_batch_horizon": (ci, [vp]),
    "mpc_batch_device_bytes": (ll, [vp]),
    "mpc_batch_state_len": (ci, [vp]),
    "mpc_batch_get_state": (ci, [vp, vp]),
    "mpc_batch_set_state": (ci, [vp, vp]),
    "mpc_batch_qp_len": (ci, [vp]),
    "mpc_batch_scale_len": (ci, [vp]),
    "mpc_batch_get_qp": (ci, [vp, vp]),
    "mpc_batch_get_scale": (ci, [vp, vp]),
    "mpc_batch_get_profile": (ci, [vp, vp]),
    "mpc_batch_enable_timing": (ci, [vp]),
    "mpc_batch_kernel_times": (ci, [vp, ci, vp, vp]),
    "mpc_last_error": (text, []),
    "mpc_ctrl_create": (ci, [pvp, ci, ci, cd, ci, cd, ci, vp, vp, ci, vp, vp, vp]),
    "mpc_ctrl_destroy": (None, [vp]),
    "mpc_ctrl_step": (ci, [vp, vp, vp, vp, vp, vp]),
    "mpc_ctrl_run": (ci, [vp, vp, vp, vp, vp, vp]),
    "mpc_ctrl_reset": (ci, [vp, vp, ci, vp]),
    "mpc_ctrl_reset_device": (ci, [vp, vp, ci, vp]),
    "mpc_ctrl_set_gait": (ci, [vp, vp, vp]),
    "mpc_ctrl_set_gait_device": (ci, [vp, vp, vp]),
    "mpc_ctrl_set_solver": (ci, [vp, ci]),
    "mpc_ctrl_solver_info": (ci, [vp, vp]),
    "mpc_ctrl_solver_record": (ci, [vp, vp]),
    "mpc_ctrl_solver_forces": (ci, [vp, vp]),
    "mpc_ctrl_solver": (vp, [vp]),
    "mpc_ctrl_set_iteration": (ci, [vp, vp, vp]),
    "mpc_device_clock": (ci, [ci, ci, vp, vp]),
    "mpc_ctrl_fsm_init": (ci, [vp, vp, ci, ci, vp]),
    "mpc_ctrl_run_fsm": (ci, [vp, vp, vp, vp, vp, vp, vp]),
    "mpc_ctrl_fsm_reset": (ci, [vp, vp, ci, vp, vp]),
    "mpc_ctrl_fsm_reset_device": (ci, [vp, vp, ci, vp]),
    "mpc_ctrl_fsm_state": (ci, [vp, vp]),
    "mpc_policy_create": (ci, [pvp, ci, vp, vp, vp, vp, vp]),
    "mpc_policy_destroy": (None, [vp]),
    "mpc_policy_step": (ci, [vp, ci, vp, vp, vp, vp]),
    "mpc_policy_observations": (ci, [ci, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mpc_ctrl_estimate": (ci, [vp, vp, vp, vp]),
    "mpc_ctrl_update_estimate": (ci, [vp, vp, vp]),
    "mpc_pack_commands": (ci, [ci, vp, vp, vp, vp]),
    "mpc_pack_commands_scaled": (ci, [ci, vp, vp, vp, vp, vp, vp]),
    "mpc_ctrl_policy_observations": (ci, [vp, vp, vp, vp, vp, vp, vp]),
    "mpc_ctrl_run_fsm_estimated": (ci, [vp, vp, vp, vp, vp, vp, vp]),
    "mpc_peer_create": (ci, [pvp, ci, ci, ci, ci]),
    "mpc_peer_handle": (ci, [vp, vp]),
    "mpc_peer_connect": (ci, [vp, vp]),
    "mpc_peer_put": (ci, [vp, vp, ci, ci, vp]),
    "mpc_peer_wait": (ci, [vp, vp, vp]),
    "mpc_peer_timeouts": (ci, [vp, vp]),
    "mpc_peer_destroy": (None, [vp]),
    "mpc_peer_last_error": (text, []),
}
SYMBOLS = list(DECLS)


class MpcLibraryError(RuntimeError):
    pass


def bind(L, decls):
    for name, (restype, argtypes) in decls.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise MpcLibraryError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # The Python host hands torch device tensors to the library, so both must sit on ONE HIP runtime: torch ships its own
        # libamdhip64 and has to be loaded first -- a library that pulled in /opt/rocm's copy before `import torch` ends up
        # with a second runtime that sees no device ("mpc_batch_create: no HIP device").
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        bind(L, DECLS)
        _LIB = L
    return _LIB


def binder(decls, base=lib):
    """The lib() of a module whose entry points are `decls`: base() with them bound as well, once per loaded library object."""
    bound = None

    def module_lib():
        nonlocal bound
        L = base()
        if bound is not L:
            bind(L, decls)
            bound = L
        return L
    return module_lib


def checker(lib, last_error):
    """check(rc, what) for the entry points whose message is behind the `last_error` symbol of lib()."""
    def check(rc, what):
        if rc != MPC_OK:
            raise MpcLibraryError(f"{what} failed ({rc}): {getattr(lib(), last_error)().decode()}")
    return check


check = checker(lib, "mpc_last_error")


def finalizer(destroy, attr="_handle"):
    """A __del__ that hands the handle in `attr` to the `destroy` entry point -- unless the library was never loaded or, at interpreter
    exit, this module's globals are gone already."""
    def __del__(self):
        h = getattr(self, attr, None)
        if h and _LIB is not None:
            getattr(_LIB, destroy)(h)
            setattr(self, attr, None)
    return __del__


def host_array(t, dtype):
    """A tensor or an array of a state dict as a numpy array of ``dtype``."""
    import numpy as np
    return (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(dtype)


class DrawnRecord:
    """What the per-robot records that are drawn on the device share (``plant_rand.PlantRand``, ``friction.Friction``): the handle once a sim is
    bound, the ``ids`` argument of a draw, and the draw counters.  A subclass names itself (``WHAT``) and, for the counters, its module's ``lib``
    and ``check`` and its two entry points (``COUNTERS``); every other entry point is called by name where it is used."""

    def _bound(self):
        if self.sim is None:
            raise ValueError(f"the {self.WHAT} is not bound to a sim (bind)")
        return self._handle

    def _counters(self, which, c):
        """The get (0) or set (1) entry point of the counters on the bound handle and the array ``c``, which the caller keeps alive."""
        lib, check, *names = self.COUNTERS
        check(getattr(lib(), names[which])(self._bound(), c.ctypes.data), names[which])

    def _ids(self, ids):
        """(address, count) of a draw's ``ids``, a cuda int32 tensor or None for all ``n``."""
        if ids is None:
            return None, self.n
        import torch
        tensor_arg(ids, torch.int32, ids.numel(), "ids")
        return ids.data_ptr(), ids.numel()

    def get_counters(self):
        """How many draws each environment has made: [n] uint32.  Synchronous."""
        import numpy as np
        c = np.zeros(self.n, np.uint32)
        self._counters(0, c)
        return c

    def set_counters(self, counters):
        import numpy as np
        c = np.ascontiguousarray(counters, dtype=np.uint32)
        if c.shape != (self.n,):
            raise ValueError(f"counters: [{self.n}] expected")
        self._counters(1, c)


def need_gpu(what, *tensors):
    import torch
    if not torch.cuda.is_available():
        raise MpcLibraryError(f"{what} needs a GPU (torch.cuda.is_available() is False); no CPU fallback")
    for t in tensors:
        if not t.is_cuda:
            raise MpcLibraryError(f"{what} runs on the device: a tensor on {t.device} was given; no CPU fallback")


def tensor_arg(t, dtype, numel, name):
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if t.dtype not in dtypes or not t.is_cuda or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{name} must be a contiguous cuda {' / '.join(str(d).replace('torch.', '') for d in dtypes)} tensor with {numel} elements")
    return t


def int_array(values):
    """A C ``int`` array of ``values``, as the ``const int *`` argument of a create."""
    return C.cast((C.c_int * len(values))(*values), C.c_void_p)


def ptr_array(addresses):
    """A C array of pointers, as the ``const float *const *`` argument of a bind."""
    return C.cast((C.c_void_p * len(addresses))(*addresses), C.c_void_p)


def addresses_to_bind(tensors, bound, device, message, like=None):
    """Bind-by-pointer: the addresses of ``tensors``, for the caller to bind and keep -- or None where they are the tuple ``bound`` of the last
    bind (None: never bound), the steady state, which costs this comparison alone.  Tensors that have to be bound are checked first: float32,
    contiguous, on ``device`` and, with ``like``, shaped like their counterparts there; ``ValueError(message)`` otherwise."""
    ptrs = tuple(t.data_ptr() for t in tensors)
    if ptrs == bound:
        return None
    import torch
    for i, t in enumerate(tensors):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device or (like is not None and t.shape != like[i].shape):
            raise ValueError(message)
    return ptrs


def flag_arg(t, n, name):
    """tensor_arg for a flag array, which may be bool or uint8 (one byte either way)."""
    import torch
    return tensor_arg(t, (torch.bool, torch.uint8), n, name)


def device_of(device):
    """The torch.device a wrapper lives on: ``device``, or torch's current cuda device for None."""
    import torch
    return torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")


def device_view(ptr, shape, typestr, device):
    """A cuda tensor of ``shape`` over the device memory at ``ptr``; the memory is a handle's, so the view is valid while its owner lives."""
    import torch

    class _Array:
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}
    return torch.as_tensor(_Array(), device=device)


def stream(device):
    """The raw handle of torch's current stream on `device`: what every stream-ordered entry point takes."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def kernel_source_hash():
    """sha256 over the kernel sources (csrc/*.h, *.hip, the Makefile): what a measurement of the library is a measurement OF.  Profiles record
    it (tools/pmc_passes.sh) and bench.py quotes a profile's numbers only when it equals the tree's."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(_HERE, "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".h", ".hip")) or f == "Makefile":
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()


def device_clock(device=0, busy_ms=20):
    """(GHz, ms): the shader clock `device` sustains under one wave of dependent fp64 FMAs per SIMD (mpc_device_clock)."""
    ghz, ms = C.c_double(0.0), C.c_double(0.0)
    check(lib().mpc_device_clock(int(device), int(busy_ms), C.addressof(ghz), C.addressof(ms)), "mpc_device_clock")
    return ghz.value, ms.value
