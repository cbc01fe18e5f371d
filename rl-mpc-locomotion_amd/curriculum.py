"""A terrain curriculum on the device (csrc/mpc_curriculum.h, csrc/mpc_curriculum.hip, csrc/terrain_curriculum.h).

legged_gym's ``_update_terrain_curriculum`` restated from its published algorithm: the field is a ``TerrainGrid`` (terrain.py) of tiles ordered by
difficulty; every environment has a type (its column of tiles, fixed) and a level (its row), and when it is reset it moves up a level if the robot
walked more than half a tile from its origin, down a level if it walked less than half of what its command asked of a whole episode, and to a
uniformly drawn level once it has passed the hardest one.  The new tile's centre is written straight into the plant's origin array, so the reset
that follows puts the robot there -- in the same tick, with no host round trip::

    grid = TerrainGrid(num_levels=10, num_types=20)                        # legged_gym's layout: 1300 x 2100 nodes
    cur = TerrainCurriculum(grid, n, max_init_level=0, seed=0)
    task = BatchedRLTask(robot_type, gait_id, curriculum=cur)              # the terrain and the initial origins come from the curriculum
    PPOTrainer(task).learn(k)                                              # records carry mean_terrain_level, terrain_level_by_type

``BatchedRLTask.step`` calls ``update`` between the plant's step and the task's ``begin``: the flags are those ``begin`` is about to consume, the
commands still the finished episode's, the root states the ones before the reset.  On the first tick every flag is set while positions and commands
are zero, so neither test fires and nobody moves (legged_gym's ``init_done`` guard without a flag).

Like legged_gym, the demotion test uses the configured episode length, not the episode's own: a robot that falls early is demoted.  Unlike torch, a
position that is not finite keeps its level (terrain_curriculum.h).  The redraw is rl_task.h's counter-based generator, uniform in distribution.

The entry points need the GPU (MpcLibraryError without one) and have no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib, toy_sim
from ._lib import cd, ci, need_gpu, pvp, text, vp

# the entry points of csrc/mpc_curriculum.h (bound here, not in any other module's list; the two mpc_terrain_* ones act on the plant's handle)
DECLS = {
    "mpc_curriculum_create": (ci, [pvp, ci, ci, ci, vp, vp, vp, cd, cd, C.c_ulonglong]),
    "mpc_curriculum_destroy": (None, [vp]),
    "mpc_curriculum_bind": (ci, [vp, vp]),
    "mpc_curriculum_update": (ci, [vp, vp, vp, vp, vp]),
    "mpc_curriculum_summary": (ci, [vp, vp, vp]),
    "mpc_curriculum_levels": (ci, [vp, pvp]),
    "mpc_curriculum_counts": (ci, [vp, pvp]),
    "mpc_curriculum_last_error": (text, []),
    "mpc_terrain_origins": (ci, [vp, pvp]),
    "mpc_terrain_get_origins": (ci, [vp, vp]),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS, base=toy_sim.lib)      # the plant's lib() (its handle and mpc_terrain_last_error) with the curriculum's entry points bound
check = _lib.checker(lib, "mpc_curriculum_last_error")
check_terrain = _lib.checker(lib, "mpc_terrain_last_error")


def sim_origins(sim):
    """The origins [n, 2] float64 of a ``BatchedToySim`` with a terrain as they are on the device now, on the host (waits for the device)."""
    out = np.zeros((sim.n, 2), np.float64)
    check_terrain(lib().mpc_terrain_get_origins(sim._handle, out.ctypes.data), "mpc_terrain_get_origins")
    return out


def sim_origin_view(sim):
    """The same array as a float64 cuda tensor [n, 2] over the plant's own memory (valid while the sim lives and keeps its terrain): what
    ``TerrainCurriculum.update`` writes and the plant's next reset reads."""
    p = C.c_void_p()
    check_terrain(lib().mpc_terrain_origins(sim._handle, C.byref(p)), "mpc_terrain_origins")
    return _lib.device_view(p.value, (sim.n, 2), "<f8", sim.device)


class TerrainCurriculum:
    """Levels and types of ``n`` environments on ``grid`` (a ``terrain.TerrainGrid``).  ``levels`` [n] int32 is a cuda tensor view of the device
    array (valid while the curriculum lives), ``counts`` [n] int32 the same for the reset counters, ``types`` [n] int32 and ``levels0`` the host arrays ``grid.assign(n, max_init_level, seed)`` gave, ``origins0`` [n, 2] float64 the
    initial origins to hand to the plant, ``terrain`` the grid's ``Terrain``.  ``env_length`` (default: the grid's tile length) and
    ``episode_length_s`` (default 20.0, ``TaskConfig``'s) are the two
    thresholds' scales; ``seed`` also keys the redraw."""

    def __init__(self, grid, n, max_init_level=0, seed=0, device=None, env_length=None, episode_length_s=20.0, levels0=None, types=None):
        import torch
        need_gpu("TerrainCurriculum")
        self.grid, self.n, self.seed = grid, int(n), int(seed)
        self.device = _lib.device_of(device)
        self.num_levels, self.num_types = int(grid.num_levels), int(grid.num_types)
        self.env_length = float(grid.env_length if env_length is None else env_length)
        self.episode_length_s = float(episode_length_s)
        a_levels, a_types = grid.assign(self.n, max_init_level, seed)
        self.levels0 = np.ascontiguousarray(a_levels if levels0 is None else levels0, dtype=np.int32).reshape(-1)
        self.types = np.ascontiguousarray(a_types if types is None else types, dtype=np.int32).reshape(-1)
        if len(self.levels0) != self.n or len(self.types) != self.n:
            raise ValueError(f"levels0 and types: {self.n} entries each")
        self.tile_origins = np.ascontiguousarray(grid.tile_origins, dtype=np.float64)
        if self.tile_origins.shape != (self.num_levels, self.num_types, 2):
            raise ValueError("grid.tile_origins must be [num_levels, num_types, 2]")
        self.terrain = grid.terrain
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().mpc_curriculum_create(C.byref(self._handle), self.n, self.num_levels, self.num_types, self.tile_origins.ctypes.data,
                                              self.levels0.ctypes.data, self.types.ctypes.data, self.env_length, self.episode_length_s,
                                              self.seed & (2 ** 64 - 1)), "mpc_curriculum_create")
        self.origins0 = np.ascontiguousarray(self.tile_origins[self.levels0, self.types])
        p = C.c_void_p()
        check(lib().mpc_curriculum_levels(self._handle, C.byref(p)), "mpc_curriculum_levels")
        self.levels = _lib.device_view(p.value, (self.n,), "<i4", self.device)
        check(lib().mpc_curriculum_counts(self._handle, C.byref(p)), "mpc_curriculum_counts")
        self.counts = _lib.device_view(p.value, (self.n,), "<i4", self.device)
        self._summary = torch.zeros((2 + 2 * self.num_types,), dtype=torch.float64, device=self.device)
        self.sim = None

    __del__ = _lib.finalizer("mpc_curriculum_destroy")

    def bind(self, sim):
        """Keep the device address of ``sim``'s origin array (a ``BatchedToySim`` with this curriculum's terrain and ``n`` robots)."""
        check(lib().mpc_curriculum_bind(self._handle, sim._handle), "mpc_curriculum_bind")
        self.sim = sim                     # (the array lives as long as the sim does)

    def update(self, reset_buf, root_states, commands):
        """For the environments whose ``reset_buf`` [n] (int64) is set: the level from ``root_states`` [n, 13] and ``commands`` [n, 3] (float32), and
        the new origin into the bound plant's array.  Stream-ordered, no host synchronisation."""
        import torch
        _lib.tensor_arg(reset_buf, torch.long, self.n, "reset_buf")
        _lib.tensor_arg(root_states, torch.float32, self.n * 13, "root_states")
        _lib.tensor_arg(commands, torch.float32, self.n * 3, "commands")
        check(lib().mpc_curriculum_update(self._handle, reset_buf.data_ptr(), root_states.data_ptr(), commands.data_ptr(), _lib.stream(self.device)),
              "mpc_curriculum_update")

    def summary(self):
        """float64 [2 + 2 num_types] on the device (the same tensor on every call): n, the mean level, per type the count, per type the mean level
        (0.0 for a type without environments).  Stream-ordered."""
        check(lib().mpc_curriculum_summary(self._handle, self._summary.data_ptr(), _lib.stream(self.device)), "mpc_curriculum_summary")
        return self._summary

    @staticmethod
    def record(values, num_types):
        """``summary().tolist()`` as the two entries of a training record."""
        return {"mean_terrain_level": values[1], "terrain_level_by_type": list(values[2 + num_types:2 + 2 * num_types])}
