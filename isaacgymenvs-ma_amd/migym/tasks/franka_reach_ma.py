"""FrankaReachMA on the MI355X path: the fork's multi-arm operational-space reach task.

Reference counterpart: tasks/franka_reach_MA.py.  ``numAgents`` Franka arms stand on a circle around a table and
reach for ``numTargets`` floating cubes; each arm is an agent with 6 actions (an end-effector pose delta turned into
joint torques by operational-space control) and ``10 + 3 T + 3 (A - 1)`` observations.  A control step is three
device launches on the caller's stream, with no host synchronisation (include/migym.h):

  ``mg_reach_pre``      pre_physics_step: action clamp and scaling, the fused OSC, torques into columns :6
  ``mg_sim_simulate``   gym.simulate, ``controlFrequencyInv`` times
  ``mg_reach_post``     post_physics_step and the VecTask.step tail: progress, the AND-filtered reset, observations,
                        compute_franka_reward, timeouts, the observation clamp

What differs from the reference:
  * no Franka asset is shipped: ``env.asset.modelTable`` names a JSON model table (``tools/build_models.py
    franka_panda`` writes one from the reference's URDF and meshes), or ``assetRoot`` + ``assetFileNameFranka`` a
    URDF, whose masses are then the loader's (kinematics only);
  * the arms collide with nothing (each is an independent articulation) and the cubes are task-owned state that only
    a reset moves, so ``root_states`` holds the arms alone, ``[arm_0 .. arm_{A-1}]`` per env, and the cubes live in
    ``_cubeA_state``; the -10 collision punishment reads the bound net contact force tensor and is live only with
    forces written into it;
  * ``controlType: osc`` only; ``task.randomize`` and the CPU host pipeline are not built for this task.
"""
from __future__ import annotations

import os

import torch

from .. import _abi
from .. import model as M
from .. import taskdefs
from .base.simulate_task import SimulateTask, state_tensors

_TASKS_DIR = os.path.dirname(os.path.abspath(__file__))


def _load_model(env) -> M.ModelSpec:
    """the arm's model table from env.asset: a JSON table (modelTable) or a URDF (assetRoot + assetFileNameFranka)"""
    asset = env.get("asset", {}) or {}
    tried = []
    table = asset.get("modelTable")
    if table:
        tried.append(str(table))
        if os.path.isfile(table):
            return M.load_json(table)
    name = asset.get("assetFileNameFranka")
    if name:
        root = asset.get("assetRoot", "../../assets")
        path = os.path.join(root if os.path.isabs(root) else os.path.join(_TASKS_DIR, root), name)
        tried.append(path)
        if os.path.isfile(path):
            return M.load_urdf(path, "franka_panda", fix_base=True)
    raise FileNotFoundError(
        "FrankaReachMA: no Franka model found (tried " + (", ".join(tried) or "nothing: env.asset is empty") +
        ").  No Franka asset ships with this package: set env.asset.modelTable to a JSON model table -- "
        "`python tools/build_models.py franka_panda` writes one from the reference's URDF and meshes -- or "
        "env.asset.assetRoot / assetFileNameFranka to the URDF (kinematics only: its masses are the loader's)")


class FrankaReachMA(SimulateTask):
    """``reset_idx(agent_ids)`` (franka_reach_MA.py:616-679): the envs whose agents are all listed (bincount(agent_ids
    // A) >= A, a repeated id counting twice) get new cubes, DOF state, targets and zero actuation, and their progress
    / reset cleared; a partial list resets nothing.  ``set_reset_noise``: per-env U(0,1) rows (N, 3 T + 9) = [z of each
    cube (T) | xy of each cube (2 T) | DOF noise (9)], the reference's draw order (franka_reach_MA.py:692, 696, 631)."""
    task_name = "FrankaReachMA"
    entry = "mg_reach"

    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture=False,
                 force_render=False):
        env = cfg["env"]
        self.control_type = env.get("controlType", "osc")
        if self.control_type not in ("osc", "joint_tor"):   # franka_reach_MA.py:66-67
            raise ValueError("Invalid control type specified. Must be one of: {osc, joint_tor}")
        if self.control_type != "osc":
            raise ValueError("controlType 'joint_tor' is not supported: the reference's own path broadcasts the "
                             "7 effort limits against 6 action columns and cannot run; use 'osc'")
        if float(env.get("frankaPositionNoise", 0.0)) > 0 or float(env.get("frankaRotationNoise", 0.0)) > 0:
            raise NotImplementedError("frankaPositionNoise / frankaRotationNoise > 0 are not implemented "
                                      "(franka_reach_MA.py:402-407 raises too)")
        self._refuse_randomize(cfg)
        A, T = taskdefs.reach_counts(env)
        env["numAgents"] = A
        self.num_targets = T
        self.max_episode_length = env["episodeLength"]
        self.action_scale = env.get("actionScale", 1.0)
        self.start_position_noise = env.get("startPositionNoise", 0.0)
        self.start_rotation_noise = env.get("startRotationNoise", 0.0)
        self.franka_dof_noise = env.get("frankaDofNoise", 0.0)
        env["numObservations"] = 10 + 3 * T + 3 * (A - 1)   # franka_reach_MA.py:75-79
        env["numActions"] = 6
        self.up_axis, self.up_axis_idx = "z", 2
        self.cubeA_size = taskdefs.REACH_CUBE_SIZE
        self._loaded_spec = _load_model(env)
        super().__init__(cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture,
                         force_render)
        # reset every env, then one observation pass (franka_reach_MA.py:222-226: reset_idx(all), _refresh())
        self.reset_idx(torch.arange(self.num_actors, device=self.device))
        self.compute_observations()

    # ---------------------------------------------------------------------------------- setup
    def create_sim(self):
        base = self._loaded_spec
        self.model_spec = spec = taskdefs.reach_spec(base)
        self.reach_params = rp = taskdefs.reach_params(self.cfg, base)
        self.task_params = None   # no fused-kernel task: mg_reach_params instead
        N, A, T = self.num_envs, self.num_agents, self.num_targets
        self.num_dof = self.num_franka_dofs = nd = spec.num_dofs
        self.num_bodies = self.num_franka_bodies = nb = len(spec.bodies)
        self.num_dofs = A * nd   # DOFs per env, as the reference counts them
        self.num_actors = n = N * A
        max_contacts = taskdefs.TASK_INFO["FrankaReachMA"][5]
        self.sim_params = taskdefs.sim_params(self.cfg, max_contacts, A)
        dev, f = self.device, torch.float32
        # root rows [arm_0 .. arm_{A-1}] per env on the reference's circle (franka_reach_MA.py:414-420)
        pos, rot = taskdefs.franka_start_poses(A)
        row = torch.zeros((A, 13), dtype=f)
        row[:, 0:2], row[:, 2], row[:, 3:7] = pos, taskdefs.TASK_INFO["FrankaReachMA"][4], rot
        self.root_states = row.repeat(N, 1).to(dev).contiguous()
        self._root_state = self.root_states.view(N, A, 13)
        self.initial_root_states = self.root_states.clone()
        self.dof_state = torch.zeros((n * nd, 2), device=dev, dtype=f)
        self._dof_state = self.dof_state.view(N, A * nd, 2)
        self._q, self._qd = self._dof_state[..., 0], self._dof_state[..., 1]
        self.dof_pos, self.dof_vel = self.dof_state.view(n, nd, 2)[..., 0], self.dof_state.view(n, nd, 2)[..., 1]
        self.dof_actuation = torch.zeros((n * nd,), device=dev, dtype=f)
        self.dof_targets = torch.zeros((n * nd,), device=dev, dtype=f)
        self._effort_control = self.dof_actuation.view(N, A * nd)
        self._pos_control = self.dof_targets.view(N, A * nd)
        self._arm_control = self._effort_control.view(-1, nd)[:, :7]
        self._gripper_control = self._pos_control.view(-1, nd)[:, -2:]
        self.rigid_body_states = torch.zeros((n * nb, 13), device=dev, dtype=f)
        self._rigid_body_state = self.rigid_body_states.view(N, A * nb, 13)
        rb = self.rigid_body_states.view(N, A, nb, 13)
        self.handles = {"base": [k * nb + spec.body_index("panda_link0") for k in range(A)],
                        "hand": [k * nb + rp.hand_body for k in range(A)],
                        "grip_site": [k * nb + rp.eef_body for k in range(A)]}
        self._eef_state = rb[:, :, rp.eef_body]
        self._base_state = rb[:, :, spec.body_index("panda_link0")]
        self.net_contact_force_tensor = torch.zeros((n * nb, 3), device=dev, dtype=f)
        self._contact_forces = self.net_contact_force_tensor.view(N, A * nb, 3)
        self._hands_contact_forces = self.net_contact_force_tensor.view(N, A, nb, 3)[:, :, rp.hand_body]
        self._cubeA_state = torch.zeros((N, T, 13), device=dev, dtype=f)
        self._init_cubeA_state = torch.zeros((N, T, 13), device=dev, dtype=f)
        lo, hi = [x.lower for x in spec.nodes[1:]], [x.upper for x in spec.nodes[1:]]
        self.franka_dof_lower_limits = self.dof_limits_lower = torch.tensor(lo, device=dev, dtype=f)
        self.franka_dof_upper_limits = self.dof_limits_upper = torch.tensor(hi, device=dev, dtype=f)
        self._franka_effort_limits = torch.tensor([x.effort_limit for x in base.nodes[1:]], device=dev, dtype=f)
        self.franka_default_dof_pos = torch.tensor(taskdefs.FRANKA_DEFAULT_DOF_POS, device=dev, dtype=f)
        self.kp = torch.tensor(list(rp.kp), device=dev, dtype=f)
        self.kd = torch.tensor(list(rp.kd), device=dev, dtype=f)
        self.kp_null = torch.tensor(list(rp.kp_null), device=dev, dtype=f)
        self.kd_null = torch.tensor(list(rp.kd_null), device=dev, dtype=f)
        self.cmd_limit = torch.tensor(list(rp.cmd_limit), device=dev, dtype=f).unsqueeze(0)
        v = _abi.StateViews()
        v.root_states, v.dof_state = _abi.ptr(self.root_states), _abi.ptr(self.dof_state)
        v.dof_actuation, v.dof_targets = _abi.ptr(self.dof_actuation), _abi.ptr(self.dof_targets)
        v.rigid_body_states = _abi.ptr(self.rigid_body_states)
        v.net_contact_forces = _abi.ptr(self.net_contact_force_tensor)
        self._create_sim_handle(spec, v)
        rv = _abi.ReachViews()
        rv.cube_states, rv.init_cube_states = _abi.ptr(self._cubeA_state), _abi.ptr(self._init_cubeA_state)
        rv.dof_targets, rv.dof_actuation = _abi.ptr(self.dof_targets), _abi.ptr(self.dof_actuation)
        self._bind_task(rp, rv, noise_shape=(N, 3 * T + 9))

    def render_boxes(self):
        """the target cubes, as the renderer's extra boxes"""
        h = 0.5 * float(self.cubeA_size)
        half = torch.full((self.num_envs, self.num_targets, 3), h, device=self.device, dtype=torch.float32)
        return torch.cat([self._cubeA_state[..., 0:7], half], dim=-1).contiguous()

    env_state_tensors = state_tensors(drop=("sensor_tensor", "dof_force_tensor"),
                                      add=("dof_targets", "rigid_body_states", "net_contact_force_tensor",
                                           "_cubeA_state", "_init_cubeA_state"))

    def compute_observations(self):
        """One observation pass on the current state without stepping (the reference's _refresh +
        compute_observations at the end of __init__): ``mg_reach_post`` on saved counters, so only obs_buf changes."""
        keep = [t.clone() for t in (self.rew_buf, self.reset_buf, self.progress_buf, self.timeout_buf)]
        self.reset_buf.zero_()
        tb = self._tb
        self._obs_actions = torch.zeros((self.num_actors, self.num_actions), device=self.device)
        tb.actions, tb.noise, tb.out_pack = self._obs_actions.data_ptr(), _abi.ptr(self._noise), None
        tb.step_counter = self.control_steps
        _abi.check(self._post(self.sim, self._params_ref, self._views_ref, _abi.C.byref(tb), None, self._stream()),
                   self._lib)
        for t, k in zip((self.rew_buf, self.reset_buf, self.progress_buf, self.timeout_buf), keep):
            t.copy_(k)
        return self.obs_buf

    @property
    def states(self):
        """the reference's ``states`` dict (franka_reach_MA.py:519-555): views of the task's tensors, and the nearest
        cube of each agent computed on access (the step computes its own in the kernel)"""
        c, a = self._cubeA_state[:, :, :3], self._eef_state[:, :, :3]
        rel = c.unsqueeze(1) - a.unsqueeze(2)
        ids = torch.argmin(rel.norm(dim=-1), dim=-1)
        env = torch.arange(ids.shape[0], device=ids.device).unsqueeze(-1).expand(ids.shape)
        out = {
            "cubeA_size": torch.ones(self.num_envs, 1, device=self.device) * self.cubeA_size,
            "q": self._q[:, :], "q_gripper": self._q[:, -2:],
            "eef_pos": self._eef_state[:, :, :3], "eef_quat": self._eef_state[:, :, 3:7],
            "eef_vel": self._eef_state[:, :, 7:],
            "cubeA_quat": self._cubeA_state[:, :, 3:7], "cubeA_pos": self._cubeA_state[:, :, 0:3],
            "cubeA_pos_min_relative": c[env, ids] - a, "nearest_cubeA_ids": ids,
            "base_pos": self._base_state[:, :, :3], "base_quat": self._base_state[:, :, 3:7],
        }
        if self.num_targets == self.num_agents:
            out["cubeA_pos_relative"] = c - a
        return out
