"""The MPC part of the RL task's step, on device tensors.

Mirror of what ``VecTask.pre_physics_step`` / ``reset_idx`` do when ``Parameters.bridge_MPC_to_RL`` is set
(RL_Environment/tasks/aliengo.py:227-263 and :321-334, same in a1.py / go1.py): rescale the policy's actions to MPC weights,
run ``controller.run`` for every environment, and reset the controllers of the environments that are being reset.  The
reference copies four tensors to the host and loops over Python controllers; here nothing leaves the GPU.  The simulator
calls themselves (``gym.set_dof_actuation_force_tensor`` ...) stay with the caller: Isaac Gym is not part of this package.

``post_physics_step`` is the other half of the tick (vec_task.py:326-337, aliengo.py:273-349): episode counter, time-outs, resets with fresh
commands, observations, reward -- two kernels of rl_task.py on the caller's tensors, again with nothing leaving the GPU.
"""
from .locomotion import BatchedLocomotion
from .weight_policy import MPC_PARAM_CONST, MPC_PARAM_SCALE


class MpcEnvBridge:
    def __init__(self, robot_type, gait_id, horizon=10, controller_dt=0.01, flat_ground=False, device=None,
                 param_scale=MPC_PARAM_SCALE, param_const=MPC_PARAM_CONST, task_cfg=None):
        import numpy as np
        import torch
        self.ctl = BatchedLocomotion(robot_type, gait_id, horizon=horizon, controller_dt=controller_dt, flat_ground=flat_ground, device=device)
        self.device, self.n = self.ctl.device, self.ctl.n
        self._scale = np.ascontiguousarray(param_scale, dtype=np.float32)       # Parameters.MPC_param_scale
        self._const = np.ascontiguousarray(param_const, dtype=np.float32)       # Parameters.MPC_param_const
        if self._scale.shape != (12,) or self._const.shape != (12,):
            raise ValueError("param_scale / param_const: twelve entries each (Parameters.py:25-33)")
        self._cmd = torch.zeros((self.n, 16), dtype=torch.float32, device=self.device)
        self._task_cfg, self.task = task_cfg, None      # rl_task.TaskPostPhysics, made by the first post_physics_step

    def pre_physics_step(self, actions, dof_state, root_states, commands):
        """actions [N,12] in [-1,1], dof_state [N*12,2] (or [N,12,2]), root_states [N,13], commands [N,3] -> torques [N,12]
        (aliengo.py:237-258).  The weights are ``actions * scale + const`` exactly as there (torch.mul(...).add(...): a float32 product, then a
        float32 sum), formed and packed with the commands into the controllers' command record by ONE kernel (mpc_pack_commands_scaled; five torch
        launches until round 5 -- tests/test_controller.py::test_env_bridge_equals_manual_composition holds the two bit-identical)."""
        import torch
        from . import _lib
        actions = actions.to(self.device, torch.float32).contiguous()
        commands = commands.to(self.device, torch.float32).contiguous()
        if actions.numel() != self.n * 12 or commands.numel() != self.n * 3:
            raise ValueError("actions [N, 12] and commands [N, 3] expected")
        stream = _lib.stream(self.device)
        _lib.check(_lib.lib().mpc_pack_commands_scaled(self.n, commands.data_ptr(), actions.data_ptr(), self._scale.ctypes.data, self._const.ctypes.data,
                                                       self._cmd.data_ptr(), stream), "mpc_pack_commands_scaled")
        return self.ctl.run(dof_state.reshape(self.n, 12, 2).contiguous(), root_states.contiguous(), self._cmd)

    def reset_idx(self, env_ids):
        """``for idx in env_ids: self.controllers[idx].reset()`` (aliengo.py:330-334)."""
        if len(env_ids):
            self.ctl.reset(env_ids)

    def post_physics_step(self, actions, torques, dof_state, root_states, contact_forces=None, base_index=0, knee_indices=None, hip_indices=None,
                          fell=None, reset_simulator=None):
        """The tick after ``gym.simulate`` (vec_task.py:326-337 with aliengo.py:273-349) -> (obs_buf, rew_buf, reset_buf, time_outs).  The task's
        buffers live in ``self.task`` (rl_task.TaskPostPhysics, configured by the constructor's ``task_cfg``): pass ``self.task.commands`` to
        ``pre_physics_step``.  The controllers of the environments being reset are reset here; ``reset_simulator(ids)`` is called in between
        with the device id array (int32 [N]: r where environment r is being reset, -1 elsewhere -- no count reaches the host) for the caller
        to reset its simulator, after which the caller's dof_state / root_states must hold the new state.  Contacts: rl_task.TaskPostPhysics.finish."""
        if self.task is None:
            from .rl_task import TaskPostPhysics
            self.task = TaskPostPhysics(self.n, self._task_cfg, device=self.device)
        ids = self.task.begin()
        self.ctl.reset(ids)
        if reset_simulator is not None:
            reset_simulator(ids)
        obs, rew, reset = self.task.finish(root_states, dof_state, actions, torques, contact_forces=contact_forces, base_index=base_index,
                                           knee_indices=knee_indices, hip_indices=hip_indices, fell=fell)
        return obs, rew, reset, self.task.timeout_buf
