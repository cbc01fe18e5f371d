"""Terrain height-scan observations on the device (csrc/mpc_height_scan.h, csrc/mpc_height_scan.hip, csrc/height_scan.h).

legged_gym's measured heights restated from its published algorithm (``_init_height_points``, ``_get_heights``, ``quat_apply_yaw``): a grid of
points around the base, rotated by the base's yaw, looked up in the plant's height field (the lowest of three nodes of the cell), and turned into
``clip(root_z - offset - h, -clip, clip) * scale``.  One kernel writes a WIDE observation row per environment -- the task's own columns copied, the
scan values, zeros up to the next multiple of 16 (the policy kernels take input widths that are multiples of 16)::

    scan = HeightScan(n)                                                   # legged_gym's 17 x 11 points: 187 values
    task = BatchedRLTask(robot_type, gait_id, terrain=terrain, height_scan=scan)      # or curriculum=...; num_obs = 48 + 187 + 5 = 240
    PPOTrainer(task).learn(k)                                              # the networks, the storage and the normaliser take num_obs from the task

A caller with a simulator of its own (``MpcEnvBridge``) binds the scan to a ``BatchedToySim`` that holds the terrain and calls ``measure`` on its own
root states and observation buffer.

Unlike legged_gym, which measures before ``reset_idx``, the scan of a tick reads the root state after the reset, the one the task's ``finish`` reads;
and positions that are not finite are clamped onto the field (height_scan.h).

The entry points need the GPU (MpcLibraryError without one) and have no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib, toy_sim
from ._lib import cd, ci, need_gpu, pvp, text, vp

MAX_POINTS = 208
# legged_gym's measured_points_x / measured_points_y
POINTS_X = (-0.8, -0.7, -0.6, -0.5, -0.4, -0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)
POINTS_Y = (-0.5, -0.4, -0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5)

# the entry points of csrc/mpc_height_scan.h (bound here, not in any other module's list)
DECLS = {
    "mpc_hscan_create": (ci, [pvp, ci, ci, vp, cd, cd, cd, cd]),
    "mpc_hscan_destroy": (None, [vp]),
    "mpc_hscan_bind": (ci, [vp, vp]),
    "mpc_hscan_run": (ci, [vp, vp, vp, ci, vp, vp, vp]),
    "mpc_hscan_width": (ci, [ci, ci]),
    "mpc_hscan_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS, base=toy_sim.lib)      # the plant's lib() (its handle is what bind takes) with the scan's entry points bound
check = _lib.checker(lib, "mpc_hscan_last_error")


def height_points(points_x=POINTS_X, points_y=POINTS_Y):
    """legged_gym's ``_init_height_points``: float32 [len(x) * len(y), 2], point ``i * len(y) + j`` is ``(x[i], y[j])``."""
    x, y = np.asarray(points_x, np.float32).reshape(-1), np.asarray(points_y, np.float32).reshape(-1)
    gx, gy = np.meshgrid(x, y, indexing="ij")
    return np.ascontiguousarray(np.stack([gx.reshape(-1), gy.reshape(-1)], -1), dtype=np.float32)


def padded_width(in_width, num_points):
    """The wide row's length, ``mpc_hscan_width``: ``in_width + num_points`` rounded up to a multiple of 16 (needs no device)."""
    w = lib().mpc_hscan_width(int(in_width), int(num_points))
    if w < 0:
        check(w, "mpc_hscan_width")
    return w


class HeightScan:
    """The scan of ``n`` environments at the points ``meshgrid(points_x, points_y)`` (metres, in the base's yaw frame; ``points`` float32 [P, 2],
    P = ``num_points`` <= 208).  ``offset``, ``clip``, ``scale`` are legged_gym's 0.5, 1.0 and ``obs_scales.height_measurements`` = 5.0;
    ``obs_clip`` is the task's ``clip_observations`` (``TaskConfig``'s default), applied last as the task applies it to its own columns."""

    def __init__(self, n, points_x=POINTS_X, points_y=POINTS_Y, offset=0.5, clip=1.0, scale=5.0, device=None, obs_clip=5.0):
        self.n = int(n)
        self.points = height_points(points_x, points_y)
        self.num_points = len(self.points)
        if not 1 <= self.num_points <= MAX_POINTS:
            raise ValueError(f"{self.num_points} points: 1 .. {MAX_POINTS} fit the padded observation row")
        self.offset, self.clip, self.scale, self.obs_clip = float(offset), float(clip), float(scale), float(obs_clip)
        import torch
        need_gpu("HeightScan")
        self.device = _lib.device_of(device)
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().mpc_hscan_create(C.byref(self._handle), self.n, self.num_points, self.points.ctypes.data, self.offset, self.clip, self.scale,
                                         self.obs_clip), "mpc_hscan_create")
        self.sim = None

    __del__ = _lib.finalizer("mpc_hscan_destroy")

    def width(self, in_width):
        """The wide row's length for a narrow row of ``in_width`` columns."""
        return padded_width(in_width, self.num_points)

    def bind(self, sim):
        """Keep ``sim``'s height field and the device address of its origin array (a ``BatchedToySim`` with a terrain and ``n`` robots).  Bind again
        after the sim's terrain is attached again."""
        check(lib().mpc_hscan_bind(self._handle, sim._handle), "mpc_hscan_bind")
        self.sim = sim                     # (the arrays live as long as the sim does)

    def measure(self, root_states, obs_in, out=None, heights=None):
        """``root_states`` [n, 13] and ``obs_in`` [n, in_width] (contiguous cuda float32) -> ``out`` [n, width(in_width)]: ``obs_in``'s columns, the
        ``num_points`` scan values, the zero pad.  ``heights`` [n, num_points] receives the measured heights in metres when given.  ``out`` is
        allocated when it is None.  Stream-ordered, no host synchronisation."""
        import torch
        _lib.tensor_arg(root_states, torch.float32, self.n * 13, "root_states")
        if obs_in.dim() != 2 or obs_in.shape[0] != self.n:
            raise ValueError(f"obs_in: [{self.n}, in_width] expected")
        in_width = int(obs_in.shape[1])
        _lib.tensor_arg(obs_in, torch.float32, self.n * in_width, "obs_in")
        w = self.width(in_width)
        if out is None:
            out = torch.empty((self.n, w), dtype=torch.float32, device=self.device)
        _lib.tensor_arg(out, torch.float32, self.n * w, "out")
        if heights is not None:
            _lib.tensor_arg(heights, torch.float32, self.n * self.num_points, "heights")
        check(lib().mpc_hscan_run(self._handle, root_states.data_ptr(), obs_in.data_ptr() if in_width else None, in_width, out.data_ptr(),
                                  None if heights is None else heights.data_ptr(), _lib.stream(self.device)), "mpc_hscan_run")
        return out
