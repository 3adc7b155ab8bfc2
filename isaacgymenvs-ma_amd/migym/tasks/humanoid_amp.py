"""HumanoidAMP on the MI355X path: the 28-DOF humanoid of Adversarial Motion Priors.

Reference counterpart: tasks/humanoid_amp.py on tasks/amp/humanoid_amp_base.py.  One free-base AMP humanoid per env
(15 bodies, 28 DOFs), 28 actions, 105 observations, and an AMP observation of ``numAMPObsSteps`` x 105 for the
discriminator.  A control step is three device launches on the caller's stream, with no host synchronisation
(include/migym.h):

  ``mg_amp_pre``        pre_physics_step: action clamp, PD targets ``offset + scale * a`` (or efforts)
  ``mg_sim_simulate``   gym.simulate, ``controlFrequencyInv`` times
  ``mg_amp_post``       post_physics_step and the VecTask.step tail: progress, the observations, reward 1,
                        compute_humanoid_reset (reset and terminate), the AMP history, timeouts, the observation clamp

Like the reference's, ``step`` resets nothing: envs are reset through ``reset_idx`` / ``reset_done()`` only
(``mg_amp_reset_idx``: all four ``stateInit`` modes, sampled on the device from the motion table of migym/motion.py),
and ``fetch_amp_obs_demo`` is one launch too (``mg_amp_obs_demo``).  The reference samples its clips with host numpy
and copies to the device on every reset; here nothing on the step or reset path runs on the host.

What differs from the reference:
  * neither the AMP humanoid nor a motion clip is shipped: ``env.asset.modelTable`` names a JSON model table
    (``tools/build_models.py amp_humanoid`` writes one from the reference's MJCF) or ``assetRoot`` + ``assetFileName``
    the MJCF; ``env.motion_file`` a clip, absolute or under ``env.asset.motionRoot``;
  * draws come from the counter RNG keyed by (seed, env, control step), not from numpy's and torch's global generators;
  * the "spherical" joints are three serial hinges here, so a reference-state init writes the reference's exp-map
    numbers into hinge angles: the pose differs from the clip's at large mixed angles;
  * ``net_contact_forces`` is the last substep's value; physics parity with PhysX is unpinned, as everywhere;
  * ``task.randomize`` and the CPU host pipeline are not built for this task.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _abi
from .. import model as M
from .. import spaces
from .. import taskdefs
from ..motion import MotionTable
from .base.simulate_task import SimulateTask, state_tensors

_TASKS_DIR = os.path.dirname(os.path.abspath(__file__))
NUM_AMP_OBS_PER_STEP = _abi.MG_AMP_OBS


def _resolve(root, name):
    return name if os.path.isabs(name) else os.path.join(root if os.path.isabs(root) else
                                                         os.path.join(_TASKS_DIR, root), name)


def _load_model(env) -> M.ModelSpec:
    """the humanoid's model table from env.asset: a JSON table (modelTable) or the MJCF (assetRoot + assetFileName)"""
    asset = env.get("asset", {}) or {}
    tried = []
    table = asset.get("modelTable")
    if table:
        tried.append(str(table))
        if os.path.isfile(table):
            return M.load_json(table)
    name = asset.get("assetFileName")
    if name and not table:   # a model table that was asked for and is missing is an error, not a reason to load an MJCF
        path = _resolve(asset.get("assetRoot", "../../assets"), name)
        tried.append(path)
        if os.path.isfile(path):
            return M.load_mjcf(path, "amp_humanoid", self_collision=True)
    raise FileNotFoundError(
        "HumanoidAMP: no AMP humanoid model found (tried " + (", ".join(tried) or "nothing: env.asset is empty") +
        ").  No AMP humanoid ships with this package: set env.asset.modelTable to a JSON model table -- "
        "`python tools/build_models.py amp_humanoid` writes one from the reference's MJCF -- or "
        "env.asset.assetRoot / assetFileName to the MJCF")


def _motion_path(env) -> str:
    asset = env.get("asset", {}) or {}
    name = env.get("motion_file", "amp_humanoid_backflip.npy")   # humanoid_amp.py:71
    path = _resolve(asset.get("motionRoot", "../../assets/amp/motions"), name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"HumanoidAMP: motion file {path} not found.  No motion clip ships with this package: "
                                "set env.motion_file to a clip in the reference's format (.npy, a plain .npz, or a "
                                ".yaml list with weights), absolute or relative to env.asset.motionRoot")
    return path


class HumanoidAMP(SimulateTask):
    task_name = "HumanoidAMP"
    entry = "mg_amp"
    acquires_dof_force = True   # humanoid_amp_base.py:88-89

    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture=False,
                 force_render=False):
        self._refuse_randomize(cfg)
        env = cfg["env"]
        self._pd_control = bool(env["pdControl"])
        self.power_scale = env["powerScale"]
        self.camera_follow = env.get("cameraFollow", False)
        plane = env.get("plane", {}) or {}
        self.plane_static_friction = plane.get("staticFriction", 1.0)
        self.plane_dynamic_friction = plane.get("dynamicFriction", 1.0)
        self.plane_restitution = plane.get("restitution", 0.0)
        self.max_episode_length = env["episodeLength"]
        self._local_root_obs = bool(env["localRootObs"])
        self._contact_bodies = list(env["contactBodies"])
        self._termination_height = env["terminationHeight"]
        self._enable_early_termination = bool(env["enableEarlyTermination"])
        self._state_init = env["stateInit"]
        self._hybrid_init_prob = env["hybridInitProb"]
        self._num_amp_obs_steps = int(env["numAMPObsSteps"])
        assert self._num_amp_obs_steps >= 2   # humanoid_amp.py:64
        env["numObservations"] = _abi.MG_AMP_OBS
        env["numActions"] = _abi.MG_AMP_DOFS
        env["numAgents"] = 1
        self.up_axis, self.up_axis_idx = "z", 2
        self._loaded_spec = _load_model(env)
        self._motion_file = _motion_path(env)
        super().__init__(cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture,
                         force_render)
        self.dt = self.control_freq_inv * float(cfg["sim"]["dt"])   # humanoid_amp_base.py:75-76
        self.num_amp_obs = self._num_amp_obs_steps * NUM_AMP_OBS_PER_STEP
        self._amp_obs_space = spaces.Box(np.ones(self.num_amp_obs) * -np.inf, np.ones(self.num_amp_obs) * np.inf)
        self._amp_obs_demo_buf = None
        self._demo_calls = 0
        self._noise_by_id = None

    # ---------------------------------------------------------------------------------- setup
    def create_sim(self):
        self.model_spec = spec = taskdefs.amp_spec(self._loaded_spec, self.cfg)
        self.amp_params = ap = taskdefs.amp_params(self.cfg, spec)
        self.task_params = None   # no fused-kernel task: mg_amp_params instead
        N = self.num_envs
        self.num_dof = nd = spec.num_dofs
        self.num_bodies = nb = len(spec.bodies)
        self.num_actors = N
        self.sim_params = taskdefs.sim_params(self.cfg, taskdefs.TASK_INFO["HumanoidAMP"][5], 1)
        dev, f = self.device, torch.float32
        self.dof_names = list(spec.dof_names)
        self._key_body_ids = torch.tensor(list(ap.key_body), device=dev, dtype=torch.long)
        names = [b.name for b in spec.bodies]
        self._contact_body_ids = torch.tensor([names.index(n) for n in self._contact_bodies], device=dev,
                                              dtype=torch.long)
        self.motor_efforts = torch.tensor(list(ap.motor_effort), device=dev, dtype=f)
        self.max_motor_effort = float(max(ap.motor_effort))
        self._pd_action_offset = torch.tensor(list(ap.pd_action_offset), device=dev, dtype=f)
        self._pd_action_scale = torch.tensor(list(ap.pd_action_scale), device=dev, dtype=f)
        self._initial_root_states = torch.tensor(list(ap.initial_root), device=dev, dtype=f).repeat(N, 1).contiguous()
        self.initial_root_states = self._initial_root_states
        self.root_states = self._root_states = self._initial_root_states.clone()
        self.dof_state = self._dof_state = torch.zeros((N * nd, 2), device=dev, dtype=f)
        self.dof_pos = self._dof_pos = self.dof_state.view(N, nd, 2)[..., 0]
        self.dof_vel = self._dof_vel = self.dof_state.view(N, nd, 2)[..., 1]
        self._initial_dof_pos = torch.tensor(list(ap.initial_dof_pos), device=dev, dtype=f).repeat(N, 1)
        self._initial_dof_vel = torch.zeros((N, nd), device=dev, dtype=f)
        self.dof_actuation = torch.zeros((N * nd,), device=dev, dtype=f)
        self.dof_targets = torch.zeros((N * nd,), device=dev, dtype=f)
        self.dof_force_tensor = torch.zeros((N, nd), device=dev, dtype=f)
        ns = max(len(spec.sensors), 1)   # the feet's force sensors (humanoid_amp_base.py:85-86, 192-198)
        self.sensor_tensor = torch.zeros((N * ns, 6), device=dev, dtype=f)
        self.vec_sensor_tensor = self.sensor_tensor.view(N, ns * 6)
        self.rigid_body_states = self._rigid_body_state = torch.zeros((N * nb, 13), device=dev, dtype=f)
        rb = self._rigid_body_state.view(N, nb, 13)
        rb[..., 6] = 1.0
        self._rigid_body_pos, self._rigid_body_rot = rb[..., 0:3], rb[..., 3:7]
        self._rigid_body_vel, self._rigid_body_ang_vel = rb[..., 7:10], rb[..., 10:13]
        self.net_contact_force_tensor = torch.zeros((N * nb, 3), device=dev, dtype=f)
        self._contact_forces = self.net_contact_force_tensor.view(N, nb, 3)
        self._terminate_buf = torch.ones(N, device=dev, dtype=torch.long)   # humanoid_amp_base.py:120
        self._amp_obs_buf = torch.zeros((N, self._num_amp_obs_steps, NUM_AMP_OBS_PER_STEP), device=dev, dtype=f)
        self._curr_amp_obs_buf = self._amp_obs_buf[:, 0]
        self._hist_amp_obs_buf = self._amp_obs_buf[:, 1:]
        lo, hi = taskdefs.dof_limits(spec)
        self.dof_limits_lower = torch.tensor(lo, device=dev, dtype=f)
        self.dof_limits_upper = torch.tensor(hi, device=dev, dtype=f)
        v = _abi.StateViews()
        v.root_states, v.dof_state = _abi.ptr(self.root_states), _abi.ptr(self.dof_state)
        v.dof_actuation = _abi.ptr(self.dof_actuation)
        v.dof_targets = _abi.ptr(self.dof_targets) if self._pd_control else None
        v.dof_force, v.sensors = _abi.ptr(self.dof_force_tensor), _abi.ptr(self.sensor_tensor)
        v.rigid_body_states = _abi.ptr(self._rigid_body_state)
        v.net_contact_forces = _abi.ptr(self.net_contact_force_tensor)
        self._create_sim_handle(spec, v)
        # the motion table (humanoid_amp.py:139-144), on the device once
        self._motion_lib = ml = MotionTable(self._motion_file, list(ap.key_body), nd)
        self._motion_frames, self._motion_index, self._motion_time = ml.to_device(dev)
        av = _abi.AmpViews()
        av.dof_targets, av.dof_actuation = _abi.ptr(self.dof_targets), _abi.ptr(self.dof_actuation)
        av.amp_obs, av.terminate = _abi.ptr(self._amp_obs_buf), _abi.ptr(self._terminate_buf)
        av.motion_frames, av.motion_index = _abi.ptr(self._motion_frames), _abi.ptr(self._motion_index)
        av.motion_time = _abi.ptr(self._motion_time)
        av.num_motions, av.num_frames = ml.num_motions(), int(self._motion_frames.shape[0])
        self._bind_task(ap, av)

    env_state_tensors = state_tensors(add=("dof_targets", "net_contact_force_tensor", "rigid_body_states",
                                           "_amp_obs_buf", "_terminate_buf"))
    env_state_scalars = SimulateTask.env_state_scalars + ("_demo_calls",)

    # ---------------------------------------------------------------------------------- hot path
    def _launch_step(self, tb, stream):
        tb.noise = None   # the step draws nothing; reset noise belongs to reset_idx
        super()._launch_step(tb, stream)

    def post_step_extras(self):
        self.extras["terminate"] = self._terminate_buf                               # humanoid_amp_base.py:384
        self.extras["amp_obs"] = self._amp_obs_buf.view(-1, self.get_num_amp_obs())  # humanoid_amp.py:93-94

    # ---------------------------------------------------------------------------------- API
    def get_num_amp_obs(self):
        return self.num_amp_obs

    @property
    def amp_observation_space(self):
        return self._amp_obs_space

    def reset_idx(self, env_ids, goal_env_ids=None):
        """reset_idx(env_ids) (humanoid_amp.py:146-256), one launch (``mg_amp_reset_idx``): per ``stateInit`` the
        listed envs get the default pose or a pose sampled from the motion table, ``progress = reset = terminate = 0``,
        their observation row and their whole AMP history."""
        super().reset_idx(env_ids)
        self._tb.noise = None

    def _reset_noise(self, n):
        noise = self._noise_by_id   # rows by list position, not by env
        if noise is not None and tuple(noise.shape) != (n, _abi.MG_AMP_NOISE_COLS):
            raise ValueError(f"reset noise must be {(n, _abi.MG_AMP_NOISE_COLS)} for this id list, "
                             f"got {tuple(noise.shape)}")
        return noise

    def set_reset_noise(self, noise):
        """Inject U(0,1) rows (n, 3) = [hybrid | motion | phase], one per id of the NEXT ``reset_idx`` calls' lists (by
        list position), instead of the device RNG; None restores the RNG."""
        if noise is not None and (noise.dim() != 2 or noise.shape[1] != _abi.MG_AMP_NOISE_COLS):
            raise ValueError(f"reset noise must be (n, {_abi.MG_AMP_NOISE_COLS}), got {tuple(noise.shape)}")
        self._noise_by_id = None if noise is None else noise.to(self.device, torch.float32).contiguous()

    def fetch_amp_obs_demo(self, num_samples, noise=None):
        """fetch_amp_obs_demo (humanoid_amp.py:108-133), one launch (``mg_amp_obs_demo``): ``(num_samples,
        numAMPObsSteps * 105)`` AMP observations of motion states drawn from the table.  ``noise``: (num_samples, 2)
        U(0,1) rows [motion | phase] instead of the device RNG."""
        num_samples = int(num_samples)
        if self._amp_obs_demo_buf is None:
            self._amp_obs_demo_buf = torch.zeros((num_samples, self._num_amp_obs_steps, NUM_AMP_OBS_PER_STEP),
                                                 device=self.device, dtype=torch.float)
        else:
            assert self._amp_obs_demo_buf.shape[0] == num_samples   # humanoid_amp.py:115
        if noise is not None:
            noise = noise.to(self.device, torch.float32).contiguous()
            if tuple(noise.shape) != (num_samples, 2):
                raise ValueError(f"demo noise must be {(num_samples, 2)}, got {tuple(noise.shape)}")
        self._demo_noise = noise
        _abi.check(self._lib.mg_amp_obs_demo(self._params_ref, self._views_ref,
                                             _abi.ptr(noise), self.seed, self._demo_calls,
                                             self._amp_obs_demo_buf.data_ptr(), num_samples, self._stream()),
                   self._lib)
        self._demo_calls += 1
        return self._amp_obs_demo_buf.view(-1, self.get_num_amp_obs())
