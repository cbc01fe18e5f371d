"""The second half of the RL task's tick, and a batched rollout environment, on the device (include/mpc_task.h, csrc/mpc_task.hip,
csrc/rl_task.h).

``MpcEnvBridge.pre_physics_step`` covers the reference's tick up to the torques.  What follows the simulator there is ``VecTask.step``
(RL_Environment/tasks/base/vec_task.py:298-339) and the task's ``post_physics_step`` (RL_Environment/tasks/aliengo.py:273-349, the same
text in a1.py / go1.py): the episode counter, the time-out flag, the reset of flagged environments with fresh commands,
``compute_robot_observations`` (the 48 observations the policy trains on), ``compute_robot_reward`` (reward and next reset flags) and
the observation clip.  Here that is two kernels, ``begin`` and ``finish``, and nothing reaches the host: where the reference takes
``reset_buf.nonzero()``, ``begin`` writes an id array with one entry per environment (its id, or -1), which every device reset entry
point of this package takes as it is because ids outside [0, n) are ignored.

    task = BatchedRLTask(robot_type, gait_id)            # MpcEnvBridge + BatchedToySim + the two kernels
    obs = task.reset()
    for _ in range(ticks):
        obs, rew, reset, extras = task.step(policy(obs))

Callers with a simulator of their own use ``MpcEnvBridge.post_physics_step`` (env_bridge.py), which runs the same two kernels on their
tensors, Isaac Gym's net contact force tensor included.

Not the reference's: commands are drawn by a counter-based generator keyed by (seed, environment, episode index), not by torch's
generator, so parity with ``torch_rand_float`` (aliengo.py:344-346) is in distribution only.

What the toy plant cannot do (BatchedRLTask only): base contact is taken to be the toy's ``fell`` flag; it has no knee or hip contacts, so
the collision term and those two reset causes never fire; and a reset puts the robot back standing on its ground (plane or terrain) -- it does not
use the randomised joint angles and velocities of aliengo.py:322-326.

Like every class here these need the GPU (MpcLibraryError without one) and have no CPU fallback.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import ci, pvp, text, vp

NUM_OBS = 48
# the order of the sum at aliengo.py:398
REWARD_TERMS = ("lin_vel_xy", "lin_vel_z", "ang_vel_xy", "ang_vel_z", "torque", "collision")
# the parts of BatchedRLTask.step, in the order it runs them (its docstring says what each one is)
STAGES = ("actions", "controller", "plant", "push", "terrain_curriculum", "begin", "episode_close", "resets", "finish", "episode_accumulate", "height_scan",
          "privileged_obs", "observation_noise")

# the entry points of include/mpc_task.h (bound here, not in _lib.SYMBOLS, which lists include/mpc_batch.h)
DECLS = {
    "mpc_task_create": (ci, [pvp, ci, vp]),
    "mpc_task_destroy": (None, [vp]),
    "mpc_task_buffers": (ci, [vp, vp]),
    "mpc_task_begin": (ci, [vp, vp]),
    "mpc_task_finish": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]),
    "mpc_task_last_error": (text, []),
}
SYMBOLS = list(DECLS)
lib = _lib.binder(DECLS)               # libmpc_batch.so with the task entry points bound
check = _lib.checker(lib, "mpc_task_last_error")


class _Config(C.Structure):            # mpc_task_config
    _fields_ = [("lin_vel_scale", C.c_double), ("ang_vel_scale", C.c_double), ("dof_pos_scale", C.c_double), ("dof_vel_scale", C.c_double),
                ("rew_scale", C.c_double * 6), ("command_range", (C.c_double * 2) * 3), ("clip_observations", C.c_double),
                ("default_dof_pos", C.c_double * 12), ("max_episode_length", C.c_longlong), ("seed", C.c_ulonglong)]


class _BufferSet(C.Structure):         # mpc_task_buffer_set
    _fields_ = [(name, C.c_void_p) for name in ("d_progress", "d_reset", "d_timeout", "d_reset_ids", "d_commands", "d_obs", "d_rew")]


@dataclass
class TaskConfig:
    """cfg/task/Aliengo.yaml restated as numbers; A1.yaml and Go1.yaml carry the same values (they differ in the base's initial height only,
    which belongs to the simulator)."""
    # learn: normalisation
    lin_vel_scale: float = 1.0
    ang_vel_scale: float = 1.0
    dof_pos_scale: float = 1.0
    dof_vel_scale: float = 1.0
    # learn: reward scales, per second (multiplied by dt where they are used, aliengo.py:78-79)
    rew_lin_vel_xy: float = 1.0
    rew_ang_vel_z: float = 0.5
    rew_torque: float = -0.000025
    rew_lin_vel_z: float = -4.0
    rew_ang_vel_xy: float = -0.05
    rew_collision: float = 0.0
    # randomCommandVelocityRanges
    command_x_range: tuple = (-2.5, 2.5)
    command_y_range: tuple = (-1.0, 1.0)
    command_yaw_range: tuple = (-2.5, 2.5)
    clip_observations: float = 5.0
    clip_actions: float = 1.0
    episode_length_s: float = 20.0
    dt: float = 0.01                   # sim.dt
    # defaultJointAngles in dof order: legs x (hip 0.0, thigh 0.8, calf -1.6)
    default_dof_pos: tuple = field(default_factory=lambda: (0.0, 0.8, -1.6) * 4)
    seed: int = 0                      # of the command generator

    @property
    def max_episode_length(self):
        return int(self.episode_length_s / self.dt + 0.5)        # aliengo.py:73-74

    def reward_scales(self):
        """The six scales x dt, in REWARD_TERMS order (aliengo.py:78-79: a Python float product)."""
        per_s = dict(lin_vel_xy=self.rew_lin_vel_xy, lin_vel_z=self.rew_lin_vel_z, ang_vel_xy=self.rew_ang_vel_xy, ang_vel_z=self.rew_ang_vel_z,
                     torque=self.rew_torque, collision=self.rew_collision)
        return [float(per_s[k]) * float(self.dt) for k in REWARD_TERMS]

    def _struct(self):
        c = _Config()
        c.lin_vel_scale, c.ang_vel_scale, c.dof_pos_scale, c.dof_vel_scale = (float(self.lin_vel_scale), float(self.ang_vel_scale),
                                                                              float(self.dof_pos_scale), float(self.dof_vel_scale))
        for i, v in enumerate(self.reward_scales()):
            c.rew_scale[i] = v
        for a, rng in enumerate((self.command_x_range, self.command_y_range, self.command_yaw_range)):
            c.command_range[a][0], c.command_range[a][1] = float(rng[0]), float(rng[1])
        c.clip_observations = float(self.clip_observations)
        if len(self.default_dof_pos) != 12:
            raise ValueError("default_dof_pos: twelve joint angles")
        for i, v in enumerate(self.default_dof_pos):
            c.default_dof_pos[i] = float(v)
        c.max_episode_length = self.max_episode_length
        c.seed = int(self.seed) & (2 ** 64 - 1)
        return c


class TaskPostPhysics:
    """The task's buffers and the two kernels, for N environments.  ``commands`` [N,3], ``progress_buf``, ``reset_buf``, ``timeout_buf`` [N]
    (int64, as the reference's), ``obs_buf`` [N,48] and ``rew_buf`` [N] are public cuda tensors; a caller may overwrite ``commands``.
    ``reset_buf`` starts at 1 (vec_task.py:240): the first tick resets every environment."""

    def __init__(self, n, cfg=None, device=None):
        import torch
        _lib.need_gpu("TaskPostPhysics")
        self.device = _lib.device_of(device)
        torch.cuda.set_device(self.device)
        self.cfg = cfg if cfg is not None else TaskConfig()
        self.n = int(n)
        self._handle = C.c_void_p()
        cs = self.cfg._struct()
        check(lib().mpc_task_create(C.byref(self._handle), self.n, C.addressof(cs)), "mpc_task_create")
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.device)
        self.obs_buf, self.rew_buf = z((self.n, NUM_OBS), torch.float32), z((self.n,), torch.float32)
        self.reset_buf = torch.ones((self.n,), dtype=torch.long, device=self.device)
        self.progress_buf, self.timeout_buf = z((self.n,), torch.long), z((self.n,), torch.long)
        self.commands = z((self.n, 3), torch.float32)
        self.reset_ids = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)
        bs = _BufferSet(self.progress_buf.data_ptr(), self.reset_buf.data_ptr(), self.timeout_buf.data_ptr(), self.reset_ids.data_ptr(),
                        self.commands.data_ptr(), self.obs_buf.data_ptr(), self.rew_buf.data_ptr())
        check(lib().mpc_task_buffers(self._handle, C.addressof(bs)), "mpc_task_buffers")

    __del__ = _lib.finalizer("mpc_task_destroy")

    def begin(self):
        """vec_task.py:326 and aliengo.py:274-278, :344-349: ``timeout_buf``, ``progress_buf += 1``, and for the environments whose ``reset_buf``
        is set fresh ``commands`` and ``progress_buf = 0``.  Returns ``reset_ids`` [N] int32 (r where environment r is being reset, -1 elsewhere)
        for the device reset entry points; stream-ordered, no host synchronisation."""
        check(lib().mpc_task_begin(self._handle, _lib.stream(self.device)), "mpc_task_begin")
        return self.reset_ids

    def finish(self, root_states, dof_state, actions, torques, contact_forces=None, base_index=0, knee_indices=None, hip_indices=None, fell=None):
        """compute_observations + compute_reward + the clip into ``obs_buf``, ``rew_buf``, ``reset_buf``.  root_states [N,13], dof_state [N*12,2],
        actions [N,12], torques [N,12]: contiguous cuda float32.  contact_forces [N,bodies,3] with base_index, knee_indices [4], hip_indices [4]
        is Isaac Gym's net contact force tensor; fell [N] (bool / uint8) is the toy plant's flag, taken as base contact."""
        import torch
        n = self.n
        for name, t, numel in (("root_states", root_states, n * 13), ("dof_state", dof_state, n * 24), ("actions", actions, n * 12), ("torques", torques, n * 12)):
            _lib.tensor_arg(t, torch.float32, numel, name)
        cf_ptr, bodies, knee, hip = None, 0, None, None
        if contact_forces is not None:
            if contact_forces.dim() != 3 or contact_forces.shape[0] != n or contact_forces.shape[2] != 3:
                raise ValueError("contact_forces: [N, bodies, 3] expected")
            bodies = int(contact_forces.shape[1])
            _lib.tensor_arg(contact_forces, torch.float32, n * bodies * 3, "contact_forces")
            if knee_indices is None or hip_indices is None:
                raise ValueError("contact_forces need knee_indices and hip_indices")
            knee = np.ascontiguousarray(knee_indices.cpu().numpy() if hasattr(knee_indices, "cpu") else knee_indices, dtype=np.int32).reshape(-1)
            hip = np.ascontiguousarray(hip_indices.cpu().numpy() if hasattr(hip_indices, "cpu") else hip_indices, dtype=np.int32).reshape(-1)
            if len(knee) != 4 or len(hip) != 4:
                raise ValueError("knee_indices and hip_indices: four body indices each")
            cf_ptr = contact_forces.data_ptr()
        fell_ptr = None if fell is None else _lib.flag_arg(fell, n, "fell").data_ptr()
        check(lib().mpc_task_finish(self._handle, root_states.data_ptr(), dof_state.data_ptr(), actions.data_ptr(), torques.data_ptr(), cf_ptr, bodies,
                                    int(base_index), None if knee is None else knee.ctypes.data, None if hip is None else hip.ctypes.data, fell_ptr,
                                    _lib.stream(self.device)), "mpc_task_finish")
        return self.obs_buf, self.rew_buf, self.reset_buf


class BatchedRLTask:
    """``VecTask.step`` / ``reset`` for N robots on the toy plant: MpcEnvBridge (actions -> torques), BatchedToySim (the simulator), and
    the two task kernels.  ``terrain`` / ``origin`` put the robots on a height field (BatchedToySim).  ``curriculum`` (a
    ``curriculum.TerrainCurriculum`` for as many environments; not together with ``terrain`` or ``origin``): the terrain and the initial origins are
    the curriculum's, and every reset moves the robot to the tile its new level names.  ``height_scan`` (a ``height_scan.HeightScan`` for as many
    environments; needs ``terrain`` or ``curriculum``): ``obs_buf`` becomes the task's own wide buffer [N, ``height_scan.width(48)``] -- the 48
    columns, the scan of the terrain around the base, a zero pad -- ``num_obs`` its width, and ``measured_heights`` [N, P] the heights in metres.
    ``domain_rand`` (a ``domain_rand.DomainRand`` for as many environments): while its ``enabled`` is true, noise on the actions in place of the
    clamp at the head of ``step``, a push of the base after the plant's step on push ticks, and noise on ``obs_buf``'s columns last.
    ``episode_terms`` (an ``episode_terms.EpisodeTerms`` for as many environments): the per-term episode sums are closed straight after ``begin``
    -- with a command curriculum the environments being reset also get commands from the curriculum's ranges in place of those ``begin`` drew --
    and fed after ``finish``; ``common_step_counter`` counts the task's ticks on the host and is the tick the curriculum sees.
    ``privileged_obs`` (a ``privileged_obs.PrivilegedObs`` for as many environments): one more launch per tick, after the height scan and BEFORE the
    observation noise, writes ``privileged_obs_buf`` [N, ``num_privileged_obs``] -- the noise-free row, the foot contacts, the episode phase, a zero
    pad -- which ``get_privileged_observations()`` returns; without it the three are None, as in rsl_rl.
    ``plant_rand`` (a ``plant_rand.PlantRand`` for as many environments): the sim gets a per-robot plant record (payload, motor strength, gravity)
    that its step consumes; with ``resample="once"`` every record is drawn when the task is built, with ``"reset"`` the environments being reset
    draw theirs inside the ``resets`` stage, before ``sim.reset_idx`` (the first tick resets, and so draws, every environment).  A
    ``PrivilegedObs(n, plant=True)`` shows the record to the critic and needs ``plant_rand``.
    ``friction`` (a ``friction.Friction`` for as many environments): the sim gets a per-robot Coulomb friction coefficient that its step consumes,
    and fills ``friction.contact_forces`` [N, 4, 3] and ``friction.foot_slip`` [N, 4]; with a spec whose ``resample`` is ``"once"`` every coefficient
    is drawn when the task is built; inside the ``resets`` stage, next to ``plant_rand.draw``, the environments being reset have their force and
    slip rows zeroed and, with ``"reset"``, draw their coefficient anew.
    ``reward_shaping`` (a ``reward_shaping.RewardShaping`` for as many environments): eight more reward terms by legged_gym's formulas; its episodes
    are closed inside the ``resets`` stage, before ``ctl.reset``, and one launch after the height scan (after ``finish`` without one) rewrites
    ``rew_buf`` with the fourteen terms and feeds its per-term sums.  The unit is made under the task's own ``cfg`` (``RewardShaping(n, spec, cfg=cfg)``; another one is refused), and a non-zero ``base_height`` scale on a terrain needs
    ``height_scan``.
    ``contact_terms`` (a ``contact_terms.ContactTerms`` for as many environments, made under the task's own ``cfg``; needs ``friction``): three more
    reward terms that read the plant's ground reactions and foot slides -- ``feet_slip``, ``feet_contact_forces``, ``feet_stumble`` -- inside the
    reward's clip; its episodes are closed inside the ``resets`` stage, next to ``reward_shaping.close``, and one launch right after
    ``reward_shaping.run`` (after ``finish`` without shaping) rewrites ``rew_buf`` and feeds its per-term sums.  With ``privileged=True`` (needs
    ``privileged_obs``) the privileged row is assembled into a narrow buffer of the task's own and one more launch inside the ``privileged_obs``
    stage writes ``privileged_obs_buf`` sixteen columns wider: the row, the friction coefficient, the twelve force components, three zeros.
    See the module text for what the toy cannot do."""

    def __init__(self, robot_type, gait_id, cfg=None, horizon=10, slope=None, yaw0=None, flat_ground=False, device=None, terrain=None, origin=None,
                 curriculum=None, height_scan=None, domain_rand=None, episode_terms=None, privileged_obs=None, plant_rand=None, reward_shaping=None, friction=None, contact_terms=None,
                 **bridge_args):
        import torch
        n_envs = len(np.asarray(robot_type).reshape(-1))
        cfg = cfg if cfg is not None else TaskConfig()
        # everything that can be refused is refused here, before the device is touched: one pass over the options, the first fault raises
        for unit, holds in ((plant_rand, None), (friction, None), (privileged_obs, "the privileged observations hold"), (episode_terms, "the episode terms hold"),
                            (reward_shaping, "the reward shaping holds"), (contact_terms, "the contact terms hold"), (domain_rand, None),
                            (height_scan, "the height scan holds"), (curriculum, "the curriculum holds")):
            if unit is None:
                continue
            if unit is plant_rand:         # counts its environments itself, with its payload against the masses of the robot types in use
                unit.validate(n=n_envs, robot_type=robot_type)
                continue
            if unit is friction:           # counts its environments itself, with its spec
                unit.validate(n=n_envs)
                continue
            if unit is privileged_obs and getattr(unit, "plant", False) and plant_rand is None:
                raise ValueError("privileged_obs has plant=True: the plant columns need plant_rand=")
            if unit is domain_rand:        # counts its environments itself, with its specs against the row's width and its push against the tick
                unit.validate(n=n_envs, num_obs=NUM_OBS if height_scan is None else height_scan.width(NUM_OBS), dt=cfg.dt)
                continue
            if unit is height_scan and terrain is None and curriculum is None:
                raise ValueError("height_scan measures a terrain: give terrain= or curriculum=")
            if unit is curriculum and (terrain is not None or origin is not None):
                raise ValueError("curriculum brings its own terrain and origins: terrain= / origin= exclude it")
            if unit.n != n_envs:
                raise ValueError(f"{holds} {unit.n} environments, robot_type {n_envs}")
            if unit is reward_shaping and unit.cfg != cfg:      # its dt, episode length, default_dof_pos and the six scales it re-evaluates are the task's
                raise ValueError("reward_shaping was made under another TaskConfig than the task's: RewardShaping(n, spec, cfg=cfg)")
            if unit is contact_terms and unit.cfg != cfg:        # its dt, episode length, clip_observations and the six scales it re-evaluates are the task's
                raise ValueError("contact_terms was made under another TaskConfig than the task's: ContactTerms(n, spec, cfg=cfg)")
            if unit is contact_terms and friction is None:
                raise ValueError("contact_terms reads the plant's ground reactions, foot slides and friction coefficients: give friction=")
            if unit is contact_terms and unit.privileged and privileged_obs is None:
                raise ValueError("contact_terms has privileged=True: the columns widen the privileged row of privileged_obs=")
            if unit is reward_shaping and unit.spec.base_height != 0 and height_scan is None and (terrain is not None or curriculum is not None):
                raise ValueError("reward_shaping has a base_height scale: on a terrain the base height is measured by height_scan=")
            if unit is height_scan and np.float32(unit.obs_clip) != np.float32(cfg.clip_observations):
                raise ValueError(f"the height scan clips its columns to {unit.obs_clip}, the task's clip_observations is {cfg.clip_observations}")
        if curriculum is not None:
            terrain, origin = curriculum.terrain, curriculum.origins0
        _lib.need_gpu("BatchedRLTask")
        from .env_bridge import MpcEnvBridge
        from .toy_sim import BatchedToySim
        self.cfg = cfg
        self.bridge = MpcEnvBridge(robot_type, gait_id, horizon=horizon, controller_dt=self.cfg.dt, flat_ground=flat_ground, device=device, **bridge_args)
        self.device, self.n = self.bridge.device, self.bridge.n
        self.num_envs, self.num_obs, self.num_actions = self.n, NUM_OBS, 12
        self.sim = BatchedToySim(robot_type, slope=slope, yaw0=yaw0, dt=self.cfg.dt, device=self.device, terrain=terrain, origin=origin)
        self.curriculum = curriculum
        if curriculum is not None:
            curriculum.bind(self.sim)
        self.task = TaskPostPhysics(self.n, self.cfg, device=self.device)
        t = self.task
        self.commands, self.progress_buf, self.reset_buf, self.timeout_buf = t.commands, t.progress_buf, t.reset_buf, t.timeout_buf
        self.obs_buf, self.rew_buf = t.obs_buf, t.rew_buf
        self.actions = torch.zeros((self.n, 12), dtype=torch.float32, device=self.device)
        self.torques = self.bridge.ctl.torques
        self.extras = {}
        self.height_scan = height_scan
        if height_scan is not None:
            height_scan.bind(self.sim)
            self.num_obs = height_scan.width(NUM_OBS)
            self.obs_buf = torch.zeros((self.n, self.num_obs), dtype=torch.float32, device=self.device)
            self.measured_heights = torch.zeros((self.n, height_scan.num_points), dtype=torch.float32, device=self.device)
        self.domain_rand = domain_rand
        if domain_rand is not None:
            domain_rand.bind(self.sim, dt=self.cfg.dt)
            self.num_active_obs = NUM_OBS + (height_scan.num_points if height_scan is not None else 0)      # what is not the scan's zero pad
        self.plant_rand = plant_rand
        if plant_rand is not None:         # before the privileged row binds the record
            plant_rand.bind(self.sim)
            if plant_rand.spec.resample == "once":
                plant_rand.draw()
        self.friction = friction
        if friction is not None:
            friction.bind(self.sim)
            if friction.spec is not None and friction.spec.resample == "once":
                friction.draw(resample=True)
        self.episode_terms = episode_terms
        self.reward_shaping = reward_shaping
        if reward_shaping is not None:
            reward_shaping.bind(self.sim)
        self.contact_terms = contact_terms
        if contact_terms is not None:      # after the friction has given the sim its record and its rows
            contact_terms.bind(self.sim)
            self._shaping_scales = None
            if reward_shaping is not None:                 # the reward's unclipped chain is rebuilt from the shaping unit's terms of the tick
                self._shaping_scales = reward_shaping.spec.scales(self.cfg.dt)
                self._shaping_terms = torch.zeros((self.n, len(self._shaping_scales)), dtype=torch.float32, device=self.device)  # (without a terms_buf)
        self.privileged_obs, self.privileged_obs_buf, self.num_privileged_obs = privileged_obs, None, None
        if privileged_obs is not None:
            from .privileged_obs import inverse_length, privileged_width
            privileged_obs.bind(self.sim)
            with_plant = getattr(privileged_obs, "plant", False)
            if with_plant:
                privileged_obs.bind_plant(self.sim)
            self._num_scan = height_scan.num_points if height_scan is not None else 0
            self._inv_len = inverse_length(self.cfg.max_episode_length)
            self.num_privileged_obs = privileged_width(self._num_scan, with_plant)
            self.privileged_obs_buf = torch.zeros((self.n, self.num_privileged_obs), dtype=torch.float32, device=self.device)
            if contact_terms is not None and contact_terms.privileged:     # assemble writes the narrow row, extend the wide one
                self._narrow_privileged = self.privileged_obs_buf
                self.num_privileged_obs = contact_terms.width(self.num_privileged_obs)
                self.privileged_obs_buf = torch.zeros((self.n, self.num_privileged_obs), dtype=torch.float32, device=self.device)
        self.common_step_counter = 0       # the ticks this task has stepped, counted on the host: the command curriculum's clock

    def step(self, actions, mark=None):
        """``VecTask.step`` (vec_task.py:298-339): actions [N,12] -> (obs_buf, rew_buf, reset_buf, {"time_outs": timeout_buf}).  The returned
        tensors are the task's own buffers, rewritten by the next step.  Nothing is copied to the host and nothing waits for the device.

        The tick's parts are named by ``STAGES``, in the order they run:
            actions             the clamp, or with action noise ``begin_step`` and the noise launch in its place
            controller          ``bridge.pre_physics_step``
            plant               ``sim.step``
            push                ``domain_rand.after_physics``              only while a DomainRand is enabled (it launches on push ticks)
            terrain_curriculum  ``curriculum.update``                      only with a curriculum
            begin               ``task.begin``
            episode_close       ``episode_terms.close_and_resample``       only with episode_terms
            resets              ``ctl.reset``, ``sim.reset_idx``, ``sim.flags``; with a PlantRand that resamples at reset ``plant_rand.draw`` first,
                                with a Friction ``friction.draw`` (the rows of the environments being reset zeroed; a coefficient drawn with "reset"),
                                with reward_shaping ``reward_shaping.close`` and with contact_terms ``contact_terms.close`` first
            finish              ``task.finish``; with reward_shaping and no height scan then ``reward_shaping.run``; with contact_terms then
                                ``contact_terms.run``, unless ``reward_shaping.run`` waits for the height scan
            episode_accumulate  ``episode_terms.accumulate``               only with episode_terms
            height_scan         ``height_scan.measure``                    only with a height scan; with reward_shaping then ``reward_shaping.run``
                                and with contact_terms ``contact_terms.run`` behind it
            privileged_obs      ``privileged_obs.assemble``                only with privileged_obs; with a privileged contact_terms then
                                ``contact_terms.extend``
            observation_noise   the observation-noise launch               only while a DomainRand is enabled and has observation noise
        ``mark``, when given, is called as ``mark(name)`` on the host right after each stage that ran on this tick has been launched, and not for a
        stage whose option is absent; a caller that records an event on the current stream in it times the stages (tools/rl_task_rate.py).  It must
        not synchronise, copy or launch anything itself, and it changes nothing in what the step computes or launches."""
        import torch
        sim, t = self.sim, self.task
        dr = self.domain_rand if self.domain_rand is not None and self.domain_rand.enabled else None
        if dr is None or dr.specs["actions"] is None:
            torch.clamp(actions.to(self.device, torch.float32).reshape(self.n, 12), -self.cfg.clip_actions, self.cfg.clip_actions, out=self.actions)    # :312
        if dr is not None:
            dr.begin_step()
            if dr.specs["actions"] is not None:                                                                                # :308-312, one launch
                dr.noise("actions", actions.to(self.device, torch.float32).reshape(self.n, 12).contiguous(), out=self.actions, clip=self.cfg.clip_actions,
                         tick=dr.tick)
        if mark is not None:
            mark("actions")
        self.torques = self.bridge.pre_physics_step(self.actions, sim.dof_state, sim.root_states, self.commands)                # aliengo.py:227-263
        if mark is not None:
            mark("controller")
        sim.step(self.torques)                                                                                                  # gym.simulate
        if mark is not None:
            mark("plant")
        if dr is not None:                 # legged_gym's _post_physics_step_callback: termination, reward and observations see the pushed velocity
            dr.after_physics(sim.root_states)
            if mark is not None:
                mark("push")
        if self.curriculum is not None:    # the flags begin is about to consume, the finished episode's commands, the root states before the reset
            self.curriculum.update(self.reset_buf, sim.root_states, self.commands)
            if mark is not None:
                mark("terrain_curriculum")
        ids = t.begin()                                                                                                         # :326, aliengo.py:274-278
        if mark is not None:
            mark("begin")
        et = self.episode_terms
        if et is not None:                 # close the marked episodes, decide, and put the curriculum's commands in place before finish reads them
            self.common_step_counter += 1
            et.close_and_resample(ids, self.commands, self.common_step_counter)
            if mark is not None:
                mark("episode_close")
        if self.plant_rand is not None and self.plant_rand.spec.resample == "reset":      # the new episode's plant, before the robot is put back
            self.plant_rand.draw(ids)
        if self.friction is not None:      # the reset environments' force and slip rows, and with resample "reset" the new episode's coefficient
            self.friction.draw(ids)
        rs = self.reward_shaping
        if rs is not None:                 # close the marked episodes' shaping sums
            rs.close(ids)
        ct = self.contact_terms
        if ct is not None:                 # and the contact sums; friction.draw has zeroed the marked environments' force and slip rows
            ct.close(ids)
        self.bridge.ctl.reset(ids)                                                                                              # aliengo.py:330-334
        sim.reset_idx(ids)                                                                                                      # aliengo.py:336-342
        _, fell = sim.flags()              # after the reset: a robot that has just been put back standing is not flagged a second time
        if mark is not None:
            mark("resets")
        t.finish(sim.root_states, sim.dof_state, self.actions, self.torques, fell=fell)                                         # aliengo.py:280-281, :337
        if rs is not None and self.height_scan is None:                        # the tensors finish has just read and written; no heights to wait for
            rs.run(sim.root_states, sim.dof_state, self.actions, self.commands, self.torques, fell, ids, self.reset_buf, self.progress_buf, self.rew_buf,
                   terms=self._terms_for_contact())
        if ct is not None and (rs is None or self.height_scan is None):        # right after the shaping launch, or after finish without one
            self._run_contact_terms(fell, ids)
        if mark is not None:
            mark("finish")
        if et is not None:                 # the tensors finish has just read, the same base contact
            et.accumulate(sim.root_states, self.commands, self.torques, fell)
            if mark is not None:
                mark("episode_accumulate")
        if self.height_scan is not None:   # the same post-reset root states, and the origins the curriculum has just written
            self.height_scan.measure(sim.root_states, t.obs_buf, out=self.obs_buf, heights=self.measured_heights)
            if rs is not None:             # the same tensors, and the heights in metres the scan has just measured
                rs.run(sim.root_states, sim.dof_state, self.actions, self.commands, self.torques, fell, ids, self.reset_buf, self.progress_buf, self.rew_buf,
                       heights=self.measured_heights, terms=self._terms_for_contact())
                if ct is not None:
                    self._run_contact_terms(fell, ids)
            if mark is not None:
                mark("height_scan")
        if self.privileged_obs is not None:                                    # the clean copy exists because this launch comes before the noise
            wide = ct is not None and ct.privileged
            self.privileged_obs.assemble(self.obs_buf, self.progress_buf, self._inv_len, num_scan=self._num_scan,
                                         out=self._narrow_privileged if wide else self.privileged_obs_buf)
            if wide:                                                           # the row, the friction coefficient and the ground reactions behind it
                ct.extend(self._narrow_privileged, self.privileged_obs_buf)
            if mark is not None:
                mark("privileged_obs")
        if dr is not None and dr.specs["observations"] is not None:                                                             # :331-337, in place
            dr.noise("observations", self.obs_buf, active=self.num_active_obs, clip=self.cfg.clip_observations, tick=dr.tick)
            if mark is not None:
                mark("observation_noise")
        self.extras["time_outs"] = self.timeout_buf
        return self.obs_buf, self.rew_buf, self.reset_buf, self.extras

    def _terms_for_contact(self):
        """The tensor ``reward_shaping.run`` writes its eight terms to: the user's ``terms_buf`` where set (None lets ``run`` pick it), else the task's
        own where the contact terms read them, else None."""
        if self.contact_terms is None or self.reward_shaping.terms_buf is not None:
            return None
        return self._shaping_terms

    def _run_contact_terms(self, fell, ids):
        rs = self.reward_shaping
        shaping_terms = None if rs is None else (rs.terms_buf if rs.terms_buf is not None else self._shaping_terms)
        self.contact_terms.run(self.sim.root_states, self.commands, self.torques, fell, ids, self.rew_buf, shaping_terms=shaping_terms,
                               shaping_scales=self._shaping_scales)

    def get_privileged_observations(self):
        """rsl_rl's ``VecEnv.get_privileged_observations``: ``privileged_obs_buf`` (rewritten by every step), or None without ``privileged_obs``."""
        return self.privileged_obs_buf

    def reset(self):
        """``VecTask.reset`` (vec_task.py:351-363): one step with zero actions; returns obs_buf."""
        import torch
        self.step(torch.zeros((self.n, 12), dtype=torch.float32, device=self.device))
        return self.obs_buf
