"""A batched TOY simulator on the device: N quadrupeds in Isaac Gym's tensor layout, so that the controller runs in closed loop on
the GPU with no host round trip per tick (include/mpc_sim.h, csrc/mpc_sim.hip, csrc/toy_sim.h).

Not a physics engine and no articulated body dynamics: one rigid body per robot under gravity; a leg in contact holds its foot at a
world anchor and pushes the body with the force its joint torques produce (F = -R J^-T tau), its joint angles following by inverse
kinematics; a leg whose force would pull on the ground by more than 5 N lets go; a leg in the air is three damped joints; a foot touches
down where its path crosses the ground: one plane z = gx x + gy y per robot, or a height field shared by all of them (``terrain=``,
rl_mpc_locomotion_amd.terrain, include/mpc_terrain.h).  float64 state, four substeps per tick.  Its only purpose is feedback that the
controller's own torques decide::

    sim = BatchedToySim(robot_type, slope=slopes, yaw0=yaws)
    bridge = MpcEnvBridge(robot_type, gait_id)
    for _ in range(ticks):
        torques = bridge.pre_physics_step(actions, sim.dof_state, sim.root_states, commands)
        sim.step(torques)

Like every class here it needs the GPU (MpcLibraryError without one) and has no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import cd, ci, pvp, text, vp
from .quadruped import ROBOT_TABLE64
from .terrain import DECLS as TERRAIN_DECLS

F64_LEN = 49      # per-robot state record: pos3 quat4 (xyzw) v3 w3 q12 qd12 anchor12
I32_LEN = 9       # contact4 lift4 fell

# the entry points of include/mpc_sim.h (bound here, not in _lib.SYMBOLS, which lists include/mpc_batch.h)
DECLS = {
    "mpc_sim_create": (ci, [pvp, ci, vp, ci, vp, vp, vp, cd]),
    "mpc_sim_destroy": (None, [vp]),
    "mpc_sim_size": (ci, [vp]),
    "mpc_sim_step": (ci, [vp, vp, vp, vp, vp]),
    "mpc_sim_observe": (ci, [vp, vp, vp, vp]),
    "mpc_sim_reset_device": (ci, [vp, vp, ci, vp]),
    "mpc_sim_get_state": (ci, [vp, vp, vp]),
    "mpc_sim_set_state": (ci, [vp, vp, vp]),
    "mpc_sim_flags": (ci, [vp, vp, vp, vp]),
    "mpc_sim_last_error": (text, []),
}
SYMBOLS = list(DECLS)
# libmpc_batch.so with the toy-plant entry points bound (include/mpc_terrain.h's are listed in terrain.SYMBOLS and bound here as well: they act on
# the same handle)
lib = _lib.binder({**DECLS, **TERRAIN_DECLS})
check = _lib.checker(lib, "mpc_sim_last_error")
check_terrain = _lib.checker(lib, "mpc_terrain_last_error")


class BatchedToySim:
    def __init__(self, robot_type, slope=None, yaw0=None, dt=0.01, device=None, terrain=None, origin=None):
        """robot_type [N] (rows of quadruped.ROBOT_TABLE64), slope [N,2] ground gradient (gx, gy) or None (flat), yaw0 [N] or None, dt the tick [s].
        Every robot starts standing on its ground plane with all four feet in contact (tests/toy_sim.py's ToyRobot.__init__).
        terrain: a rl_mpc_locomotion_amd.terrain.Terrain in place of the planes (not together with a non-zero slope), origin [N,2] where on
        it each robot's local (0, 0) lies (None: the terrain's own (0, 0)); the robots' coordinates and root_states stay local."""
        import torch
        if terrain is not None and slope is not None and np.any(np.asarray(slope, dtype=np.float64) != 0.0):
            raise ValueError("terrain and a non-zero slope exclude each other: the terrain replaces the plane")
        if terrain is None and origin is not None:
            raise ValueError("origin needs a terrain")
        _lib.need_gpu("BatchedToySim")
        self.device = _lib.device_of(device)
        torch.cuda.set_device(self.device)
        rt = np.ascontiguousarray(robot_type, dtype=np.int32).reshape(-1)
        self.n = len(rt)
        self.robot_type = rt
        sl = None if slope is None else np.ascontiguousarray(np.broadcast_to(np.asarray(slope, dtype=np.float64), (self.n, 2)))
        yw = None if yaw0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(yaw0, dtype=np.float64), (self.n,)))
        tab = np.ascontiguousarray(ROBOT_TABLE64, dtype=np.float64)
        self._handle = C.c_void_p()
        check(lib().mpc_sim_create(C.byref(self._handle), self.n, rt.ctypes.data, tab.shape[0], tab.ctypes.data,
                                   None if sl is None else sl.ctypes.data, None if yw is None else yw.ctypes.data, float(dt)), "mpc_sim_create")
        self.dof_state = torch.zeros((self.n * 12, 2), dtype=torch.float32, device=self.device)     # gym's dof-state tensor
        self.root_states = torch.zeros((self.n, 13), dtype=torch.float32, device=self.device)       # gym's actor root-state tensor
        self._contact = torch.zeros((self.n, 4), dtype=torch.bool, device=self.device)
        self._fell = torch.zeros((self.n,), dtype=torch.bool, device=self.device)
        self.terrain, self.origin = terrain, None
        if terrain is not None:
            self.origin = np.zeros((self.n, 2)) if origin is None else np.ascontiguousarray(np.broadcast_to(np.asarray(origin, dtype=np.float64), (self.n, 2)))
            hts = np.ascontiguousarray(terrain.heights, dtype=np.int16)
            check_terrain(lib().mpc_terrain_attach(self._handle, hts.shape[0], hts.shape[1], hts.ctypes.data, float(terrain.hscale), float(terrain.vscale),
                                                   float(terrain.x0), float(terrain.y0), self.origin.ctypes.data), "mpc_terrain_attach")
        self._observe()

    __del__ = _lib.finalizer("mpc_sim_destroy")

    def _observe(self):
        check(lib().mpc_sim_observe(self._handle, self.dof_state.data_ptr(), self.root_states.data_ptr(), _lib.stream(self.device)), "mpc_sim_observe")

    def step(self, torques):
        """One tick of every robot that has not fallen, torques [N,12] contiguous cuda float32 (FL FR RL RR x hip, thigh, calf).
        Updates dof_state and root_states in place and returns them; stream-ordered, no host synchronisation."""
        import torch
        _lib.tensor_arg(torques, torch.float32, self.n * 12, "torques")
        check(lib().mpc_sim_step(self._handle, torques.data_ptr(), self.dof_state.data_ptr(), self.root_states.data_ptr(), _lib.stream(self.device)), "mpc_sim_step")
        return self.dof_state, self.root_states

    def reset_idx(self, env_ids):
        """Re-initialise the robots `env_ids` (host list / numpy array, or a cuda tensor: then without a host round trip) and refresh the
        observation tensors; every other robot is left bit for bit as it is."""
        import torch
        if hasattr(env_ids, "is_cuda") and env_ids.is_cuda:
            d_ids = env_ids.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            ids = np.ascontiguousarray(env_ids.detach().cpu().numpy() if hasattr(env_ids, "detach") else env_ids, dtype=np.int32).reshape(-1)
            if len(ids) == 0:
                return
            d_ids = torch.from_numpy(ids).to(self.device)
        if d_ids.numel() == 0:
            return
        check(lib().mpc_sim_reset_device(self._handle, d_ids.data_ptr(), d_ids.numel(), _lib.stream(self.device)), "mpc_sim_reset_device")
        self._observe()

    def terrain_query(self, xy, normals=True):
        """Height [K] and unit normal [K,3] (None without `normals`) of the attached terrain at xy [K,2], a contiguous cuda float64 tensor of points
        in the terrain's own frame (no robot origin); stream-ordered."""
        import torch
        if xy.dtype != torch.float64 or not xy.is_cuda or not xy.is_contiguous() or xy.dim() != 2 or xy.shape[1] != 2:
            raise ValueError("xy must be a contiguous cuda float64 tensor [K, 2]")
        k = int(xy.shape[0])
        z = torch.zeros((k,), dtype=torch.float64, device=self.device)
        nrm = torch.zeros((k, 3), dtype=torch.float64, device=self.device) if normals else None
        check_terrain(lib().mpc_terrain_query(self._handle, xy.data_ptr(), k, z.data_ptr(), None if nrm is None else nrm.data_ptr(), _lib.stream(self.device)),
                      "mpc_terrain_query")
        return z, nrm

    def flags(self):
        """(contact [N,4] bool, fell [N] bool) cuda tensors of the current state (the same two tensors on every call)."""
        check(lib().mpc_sim_flags(self._handle, self._contact.data_ptr(), self._fell.data_ptr(), _lib.stream(self.device)), "mpc_sim_flags")
        return self._contact, self._fell

    def get_state(self):
        """The whole state on the host: {"f64": [N,49] float64 (pos3 quat4 v3 w3 q12 qd12 anchor12), "i32": [N,9] int32 (contact4 lift4 fell)}."""
        f = np.zeros((self.n, F64_LEN), np.float64)
        k = np.zeros((self.n, I32_LEN), np.int32)
        check(lib().mpc_sim_get_state(self._handle, f.ctypes.data, k.ctypes.data), "mpc_sim_get_state")
        return {"f64": f, "i32": k}

    def set_state(self, state):
        """Restore a state of get_state's layout and refresh the observation tensors."""
        f = np.ascontiguousarray(state["f64"], dtype=np.float64)
        k = np.ascontiguousarray(state["i32"], dtype=np.int32)
        if f.shape != (self.n, F64_LEN) or k.shape != (self.n, I32_LEN):
            raise ValueError(f"state: f64 [{self.n}, {F64_LEN}] and i32 [{self.n}, {I32_LEN}] expected")
        check(lib().mpc_sim_set_state(self._handle, f.ctypes.data, k.ctypes.data), "mpc_sim_set_state")
        self._observe()
