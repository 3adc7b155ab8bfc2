"""Anymal on the MI355X path: the PD-driven quadruped that tracks a velocity command.

Reference counterpart: tasks/anymal.py.  One free-base ANYmal C per env, 12 joints on position drives, 12 actions
(joint target offsets) and 48 observations.  A control step is three device launches on the caller's stream, with no
host synchronisation (include/migym.h):

  ``mg_anymal_pre``     pre_physics_step: action clamp, ``targets = actionScale * a + default_dof_pos``
  ``mg_sim_simulate``   gym.simulate, ``controlFrequencyInv`` times
  ``mg_anymal_post``    post_physics_step and the VecTask.step tail: progress, resets (DOF state, root row, new
                        commands), observations, compute_anymal_reward, timeouts, the observation clamp

What differs from the reference:
  * no ANYmal asset is shipped: ``env.asset.modelTable`` names a JSON model table (``tools/build_models.py anymal_c``
    writes one from the reference's URDF), or ``assetRoot`` + ``assetFileName`` the URDF itself;
  * the DOF order is the loader's (depth first in URDF order: LF, RF, LH, RH x HAA, HFE, KFE);
  * an indexed set is visible at once: a reset env is observed in its reset state;
  * ``task.randomize`` and the CPU host pipeline are not built for this task.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _abi
from .. import model as M
from .. import taskdefs
from .base.simulate_task import SimulateTask, state_tensors

_TASKS_DIR = os.path.dirname(os.path.abspath(__file__))


def _load_model(env, task="Anymal", builder="anymal_c") -> M.ModelSpec:
    """the robot's model table from env.asset: a JSON table (modelTable) or a URDF (assetRoot + assetFileName);
    ``task`` and ``builder`` (the tools/build_models.py command that writes one) name themselves in the error"""
    asset = env.get("asset", {}) or {}
    tried = []
    table = asset.get("modelTable")
    if table:
        tried.append(str(table))
        if os.path.isfile(table):
            return M.load_json(table)
    name = asset.get("assetFileName")
    if name and not table:   # a model table that was asked for and is missing is an error, not a reason to load a URDF
        root = asset.get("assetRoot", "../../assets")
        path = os.path.join(root if os.path.isabs(root) else os.path.join(_TASKS_DIR, root), name)
        tried.append(path)
        if os.path.isfile(path):
            urdf = env.get("urdfAsset", {}) or {}
            return M.load_urdf(path, "anymal_c", fix_base=bool(urdf.get("fixBaseLink", False)),
                               collapse_fixed=True, replace_cylinder_with_capsule=True, effort_limits=True)
    raise FileNotFoundError(
        f"{task}: no ANYmal model found (tried " + (", ".join(tried) or "nothing: env.asset is empty") +
        ").  No ANYmal asset ships with this package: set env.asset.modelTable to a JSON model table -- "
        f"`python tools/build_models.py {builder}` writes one from the reference's URDF -- or "
        "env.asset.assetRoot / assetFileName to the URDF")


class Anymal(SimulateTask):
    """``reset_idx(env_ids)`` (anymal.py:278-304): the listed envs get ``dof_pos = default * U(0.5, 1.5)``, ``dof_vel =
    U(-0.1, 0.1)``, the base init state, three new commands and ``progress = 0``; like the reference's, it leaves
    ``reset_buf`` of those envs at 1 (the next step's compute_reward overwrites it).  ``set_reset_noise``: per-env
    U(0,1) rows (N, 27) = [positions_offset 12 | velocities 12 | command x | y | yaw], the reference's draw order
    (anymal.py:283-301)."""
    task_name = "Anymal"
    entry = "mg_anymal"
    acquires_dof_force = True   # anymal.py:113

    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture=False,
                 force_render=False):
        self._refuse_randomize(cfg)
        env = cfg["env"]
        learn, ctl = env["learn"], env["control"]
        self.lin_vel_scale, self.ang_vel_scale = learn["linearVelocityScale"], learn["angularVelocityScale"]
        self.dof_pos_scale, self.dof_vel_scale = learn["dofPositionScale"], learn["dofVelocityScale"]
        self.action_scale = ctl["actionScale"]
        rng = env["randomCommandVelocityRanges"]
        self.command_x_range, self.command_y_range, self.command_yaw_range = rng["linear_x"], rng["linear_y"], rng["yaw"]
        plane = env.get("plane", {}) or {}
        self.plane_static_friction = plane.get("staticFriction", 1.0)
        self.plane_dynamic_friction = plane.get("dynamicFriction", 1.0)
        self.plane_restitution = plane.get("restitution", 0.0)
        b = env["baseInitState"]
        self.base_init_state = list(b["pos"]) + list(b["rot"]) + list(b["vLinear"]) + list(b["vAngular"])
        self.named_default_joint_angles = env["defaultJointAngles"]
        env["numObservations"] = _abi.MG_ANYMAL_OBS
        env["numActions"] = _abi.MG_ANYMAL_DOFS
        env["numAgents"] = 1
        # controlFrequencyInv is env.controlFrequencyInv, as VecTask reads it (vec_task.py:231): the reference never
        # reads the env.control.controlFrequencyInv of its own YAML
        self.up_axis, self.up_axis_idx = "z", 2
        self.Kp, self.Kd = ctl["stiffness"], ctl["damping"]
        self._loaded_spec = _load_model(env)
        super().__init__(cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture,
                         force_render)
        self.reset_idx(torch.arange(self.num_envs, device=self.device))   # anymal.py:146

    # ---------------------------------------------------------------------------------- setup
    def create_sim(self):
        self.model_spec = spec = taskdefs.anymal_spec(self._loaded_spec, self.cfg)
        self.anymal_params = ap = taskdefs.anymal_params(self.cfg, spec)
        self.task_params = None   # no fused-kernel task: mg_anymal_params instead
        N = self.num_envs
        self.num_dof = nd = spec.num_dofs
        self.num_bodies = nb = len(spec.bodies)
        self.num_actors = N
        learn = self.cfg["env"]["learn"]
        dt32 = float(np.float32(self.dt))   # gymapi.SimParams.dt is a C float
        self.max_episode_length_s = learn["episodeLength_s"]
        self.max_episode_length = ap.max_episode_length
        self.rew_scales = {"lin_vel_xy": learn["linearVelocityXYRewardScale"] * dt32,
                           "ang_vel_z": learn["angularVelocityZRewardScale"] * dt32,
                           "torque": learn["torqueRewardScale"] * dt32}
        self.sim_params = taskdefs.sim_params(self.cfg, taskdefs.TASK_INFO["Anymal"][5], 1)
        dev, f = self.device, torch.float32
        self.dof_names = list(spec.dof_names)
        names = [b.name for b in spec.bodies]
        self.feet_indices = torch.tensor([i for i, s in enumerate(names) if taskdefs.ANYMAL_FOOT in s], device=dev,
                                         dtype=torch.long)
        self.knee_indices = torch.tensor(list(ap.knee_body), device=dev, dtype=torch.long)
        self.base_index = int(ap.base_body)
        self.initial_root_states = torch.tensor(self.base_init_state, device=dev, dtype=f).repeat(N, 1).contiguous()
        self.root_states = self.initial_root_states.clone()
        self.dof_state = torch.zeros((N * nd, 2), device=dev, dtype=f)
        self.dof_pos = self.dof_state.view(N, nd, 2)[..., 0]
        self.dof_vel = self.dof_state.view(N, nd, 2)[..., 1]
        self.dof_actuation = torch.zeros((N * nd,), device=dev, dtype=f)
        self.dof_targets = torch.zeros((N * nd,), device=dev, dtype=f)
        self.dof_force_tensor = torch.zeros((N, nd), device=dev, dtype=f)
        self.torques = self.dof_force_tensor.view(N, nd)
        self.net_contact_force_tensor = torch.zeros((N * nb, 3), device=dev, dtype=f)
        self.contact_forces = self.net_contact_force_tensor.view(N, nb, 3)
        self.commands = torch.zeros((N, 3), device=dev, dtype=f)
        self.commands_x, self.commands_y = self.commands[..., 0], self.commands[..., 1]
        self.commands_yaw = self.commands[..., 2]
        self.default_dof_pos = torch.tensor(list(ap.default_dof_pos), device=dev, dtype=f).repeat(N, 1)
        self.gravity_vec = torch.tensor([0.0, 0.0, -1.0], device=dev, dtype=f).repeat(N, 1)
        lo, hi = taskdefs.dof_limits(spec)
        self.dof_limits_lower = torch.tensor(lo, device=dev, dtype=f)
        self.dof_limits_upper = torch.tensor(hi, device=dev, dtype=f)
        v = _abi.StateViews()
        v.root_states, v.dof_state = _abi.ptr(self.root_states), _abi.ptr(self.dof_state)
        v.dof_actuation, v.dof_targets = _abi.ptr(self.dof_actuation), _abi.ptr(self.dof_targets)
        v.dof_force = _abi.ptr(self.dof_force_tensor)
        v.net_contact_forces = _abi.ptr(self.net_contact_force_tensor)
        self._create_sim_handle(spec, v)
        av = _abi.AnymalViews()
        av.commands, av.dof_targets = _abi.ptr(self.commands), _abi.ptr(self.dof_targets)
        self._bind_task(ap, av, noise_shape=(N, _abi.MG_ANYMAL_NOISE_COLS))

    env_state_tensors = state_tensors(drop=("sensor_tensor",),
                                      add=("dof_targets", "net_contact_force_tensor", "commands"))
