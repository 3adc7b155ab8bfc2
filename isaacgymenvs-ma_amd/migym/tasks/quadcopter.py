"""Quadcopter on the MI355X path: four tilting rotors whose thrusts are forces on links.

Reference counterpart: tasks/quadcopter.py.  One free-base quadcopter per env (chassis, four arms on pitch hinges, four
rotors on roll hinges), 8 joints on position drives, 12 actions (8 joint target rates, 4 thrust rates) and 21
observations.  A control step is three device launches on the caller's stream, with no host synchronisation
(include/migym.h):

  ``mg_quadcopter_pre``    pre_physics_step: the pending resets, the action clamp, ``targets += dt 8 pi a[0:8]`` and
                           ``thrusts += dt 200 a[8:12]`` with their clamps, the force tensor's rotor rows
  ``mg_sim_simulate``      gym.simulate with link forces on (``LOCAL_SPACE``), ``controlFrequencyInv`` times
  ``mg_quadcopter_post``   post_physics_step and the VecTask.step tail: progress, observations,
                           compute_quadcopter_reward, timeouts, the observation clamp

What differs from the reference:
  * the reference writes its MJCF at run time and loads that; here ``migym.model.quadcopter_model`` builds the same
    table from the named dimensions, so the task needs no asset;
  * cylinder geoms are not collided by the step kernels: only the arm spheres touch the plane (the task resets below
    z = 0.3, so its rollouts never get there);
  * the thrusts persist over the ``controlFrequencyInv`` simulates of a control step (gym clears applied forces after
    each simulate; the reference's YAML has controlFrequencyInv 1);
  * ``apply_rigid_body_force_tensors`` puts the caller's tensor in the place of ``env.forces`` (LOCAL_SPACE only);
  * ``enableDebugVis`` is ignored; ``task.randomize`` and the CPU host pipeline are not built for this task.
"""
from __future__ import annotations

import torch

from .. import _abi
from .. import model as M
from .. import taskdefs
from .base.simulate_task import SimulateTask, state_tensors


class Quadcopter(SimulateTask):
    """``reset_idx(env_ids)`` (quadcopter.py:280-299): the listed envs get their DOF state and root row from the initial
    state, x, y += U(-1.5, 1.5), z += U(-0.2, 1.5), DOF positions U(-0.2, 0.2), velocities 0, ``reset_buf = 0`` and
    ``progress_buf = 0``.  Thrusts, forces and targets are cleared by pre_physics_step, for the envs it resets itself.
    ``set_reset_noise``: per-env U(0,1) rows (N, 11) = [x | y | z | dof position 8], the reference's draw order
    (quadcopter.py:289-294)."""
    task_name = "Quadcopter"
    entry = "mg_quadcopter"

    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture=False,
                 force_render=False):
        self._refuse_randomize(cfg)
        env = cfg["env"]
        self.max_episode_length = env["maxEpisodeLength"]
        self.debug_viz = env.get("enableDebugVis", False)   # ignored: there is no viewer
        env["numObservations"] = _abi.MG_QUAD_OBS
        env["numActions"] = _abi.MG_QUAD_ACTIONS
        env["numAgents"] = 1
        super().__init__(cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture, force_render)

    # ---------------------------------------------------------------------------------- setup
    def create_sim(self):
        self.model_spec = spec = taskdefs.quadcopter_spec(M.quadcopter_model())
        self.quadcopter_params = qp = taskdefs.quadcopter_params(self.cfg, spec)
        self.task_params = None   # no fused-kernel task: mg_quadcopter_params instead
        N = self.num_envs
        self.num_dof = self.num_dofs = nd = spec.num_dofs
        self.num_bodies = nb = len(spec.bodies)
        self.num_actors = N
        self.sim_params = taskdefs.sim_params(self.cfg, taskdefs.QUADCOPTER_MAX_CONTACTS, 1)
        dev, f = self.device, torch.float32
        self.initial_root_states = torch.tensor(list(qp.init_root), device=dev, dtype=f).repeat(N, 1).contiguous()
        self.root_states = self.initial_root_states.clone()
        self.root_positions, self.root_quats = self.root_states[:, 0:3], self.root_states[:, 3:7]
        self.root_linvels, self.root_angvels = self.root_states[:, 7:10], self.root_states[:, 10:13]
        self.dof_state = torch.zeros((N * nd, 2), device=dev, dtype=f)
        self.dof_states = self.dof_state.view(N, nd, 2)
        self.initial_dof_states = self.dof_states.clone()
        self.dof_positions, self.dof_velocities = self.dof_states[..., 0], self.dof_states[..., 1]
        self.dof_pos, self.dof_vel = self.dof_positions, self.dof_velocities
        self.dof_actuation = torch.zeros((N * nd,), device=dev, dtype=f)
        self.dof_position_targets = torch.zeros((N, nd), device=dev, dtype=f)
        self.thrusts = torch.zeros((N, 4), device=dev, dtype=f)
        self.forces = torch.zeros((N, nb, 3), device=dev, dtype=f)
        lo, hi = taskdefs.dof_limits(spec)
        self.dof_lower_limits = self.dof_limits_lower = torch.tensor(lo, device=dev, dtype=f)
        self.dof_upper_limits = self.dof_limits_upper = torch.tensor(hi, device=dev, dtype=f)
        self.dof_ranges = self.dof_upper_limits - self.dof_lower_limits
        self.thrust_lower_limits = torch.full((4,), qp.thrust_lower, device=dev, dtype=f)
        self.thrust_upper_limits = torch.full((4,), qp.thrust_upper, device=dev, dtype=f)
        v = _abi.StateViews()
        v.root_states, v.dof_state = _abi.ptr(self.root_states), _abi.ptr(self.dof_state)
        v.dof_actuation, v.dof_targets = _abi.ptr(self.dof_actuation), _abi.ptr(self.dof_position_targets)
        # gym.apply_rigid_body_force_tensors(sim, forces, None, LOCAL_SPACE) (quadcopter.py:330)
        v.rb_forces, v.rb_force_space = _abi.ptr(self.forces), _abi.MG_LOCAL_SPACE
        self.rb_forces = self.forces
        self._create_sim_handle(spec, v)
        _abi.check(self._lib.mg_sim_set_link_forces(self.sim, 1), self._lib)
        qv = _abi.QuadcopterViews()
        qv.thrusts, qv.dof_targets = _abi.ptr(self.thrusts), _abi.ptr(self.dof_position_targets)
        qv.forces = _abi.ptr(self.forces)
        self._bind_task(qp, qv, noise_shape=(N, _abi.MG_QUAD_NOISE_COLS))

    env_state_tensors = state_tensors(drop=("sensor_tensor", "dof_force_tensor"),
                                      add=("thrusts", "dof_position_targets", "forces"))

    # ---------------------------------------------------------------------------------- API
    def apply_rigid_body_force_tensors(self, forces, torques=None, space=_abi.MG_LOCAL_SPACE):
        """As VecTask's, with the caller's (N, 9, 3) tensor taking the place of ``env.forces``: every step writes the
        thrusts into its rotor rows' z components (and zeroes the rows of an env it resets), the other entries are the
        caller's.  The thrusts act along the rotors' own axes, so the space must be ``LOCAL_SPACE``."""
        if space != _abi.MG_LOCAL_SPACE:
            raise ValueError("Quadcopter: the force tensor carries the thrusts along the rotors' own z axes "
                             "(quadcopter.py:330): space must be LOCAL_SPACE")
        super().apply_rigid_body_force_tensors(forces, torques, space)
        self.forces = forces
        self._task_views.forces = forces.data_ptr()
