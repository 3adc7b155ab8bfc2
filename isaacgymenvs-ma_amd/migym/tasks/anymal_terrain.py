"""AnymalTerrain on the MI355X path: rough-terrain locomotion with a terrain curriculum.

Reference counterpart: tasks/anymal_terrain.py.  One free-base ANYmal C per env in effort mode, 12 actions (joint
target offsets of an explicit PD law), 188 observations (base velocities, gravity, commands, DOF state, 140 terrain
heights around the base, the last actions).  A control step is a fixed sequence of device launches on the caller's
stream, with no host synchronisation (include/migym.h):

  ``mg_anymal_terrain_pre``    the PD torque of one decimation step, into ``dof_actuation`` and ``torques``
  ``mg_sim_simulate``          gym.simulate on the heightfield; the pair runs ``control.decimation`` times
  ``mg_anymal_terrain_post``   post_physics_step and the VecTask.step tail: the push, termination, the 13-term reward,
                               resets with the curriculum update, the height scan, noise, ``extras["episode"]``

What differs from the reference:
  * the terrain is the heightfield itself, not a triangle mesh: vertical faces are one-cell ramps;
  * the sub-terrain functions are this package's own (migym/terrain.py), not isaacgym.terrain_utils;
  * the curriculum takes the norm of each env's own commands, not the norm over every env that resets with it;
  * per-env friction (``frictionRange``), debug visualisation and the renderer's terrain are not built;
  * ``learn.pushRobots: false`` is honoured (the reference never reads it);
  * no ANYmal asset is shipped: ``env.asset.modelTable`` names a JSON model table (``tools/build_models.py
    anymal_minimal`` writes one from the reference's URDF), or ``assetRoot`` + ``assetFileName`` the URDF itself.
"""
from __future__ import annotations

import torch

from .. import _abi
from .. import taskdefs
from ..terrain import Terrain
from .anymal import _load_model
from .base.simulate_task import SimulateTask, state_tensors


class AnymalTerrain(SimulateTask):
    """``set_reset_noise``: per-env U(0,1) rows (N, 219) = [push vx vy 2 | positions_offset 12 | velocities 12 | root x
    y 2 | command x | y | heading | observation noise 188], the reference's draw order."""
    task_name = "AnymalTerrain"
    entry = "mg_anymal_terrain"

    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture=False,
                 force_render=False):
        self._refuse_randomize(cfg)
        env = cfg["env"]
        learn, ctl, ter = env["learn"], env["control"], env["terrain"]
        if ter["terrainType"] not in ("plane", "trimesh"):
            raise NameError(f"AnymalTerrain: terrainType must be 'plane' or 'trimesh', got {ter['terrainType']!r} "
                            "(heights cannot be measured without a terrain)")
        self.custom_origins = ter["terrainType"] == "trimesh"
        self.lin_vel_scale, self.ang_vel_scale = learn["linearVelocityScale"], learn["angularVelocityScale"]
        self.dof_pos_scale, self.dof_vel_scale = learn["dofPositionScale"], learn["dofVelocityScale"]
        self.height_meas_scale = learn["heightMeasurementScale"]
        self.action_scale = ctl["actionScale"]
        rng = env["randomCommandVelocityRanges"]
        self.command_x_range, self.command_y_range, self.command_yaw_range = rng["linear_x"], rng["linear_y"], rng["yaw"]
        b = env["baseInitState"]
        self.base_init_state = list(b["pos"]) + list(b["rot"]) + list(b["vLinear"]) + list(b["vAngular"])
        self.named_default_joint_angles = env["defaultJointAngles"]
        self.decimation = int(ctl["decimation"])
        step_dt = self.decimation * cfg["sim"]["dt"]
        self.max_episode_length_s = learn["episodeLength_s"]
        self.push_interval = int(learn["pushInterval_s"] / step_dt + 0.5)
        self.push_robots = bool(learn.get("pushRobots", True))
        self.allow_knee_contacts = learn["allowKneeContacts"]
        self.Kp, self.Kd = ctl["stiffness"], ctl["damping"]
        self.curriculum = ter["curriculum"]
        self.common_step_counter = 0
        env["numObservations"] = _abi.MG_ANYMAL_TERRAIN_OBS
        env["numActions"] = _abi.MG_ANYMAL_DOFS
        env["numAgents"] = 1
        self.up_axis, self.up_axis_idx = "z", 2
        self._loaded_spec = _load_model(env, "AnymalTerrain", "anymal_minimal")
        super().__init__(cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture,
                         force_render)
        self.extras["episode"] = {}
        # anymal_terrain.py:160: the constructor's reset leaves the terrain levels alone (init_done)
        self.reset_idx(torch.arange(self.num_envs, device=self.device), update_levels=False)

    # ---------------------------------------------------------------------------------- setup
    def create_sim(self):
        cfg, env = self.cfg, self.cfg["env"]
        ter = env["terrain"]
        self.model_spec = spec = taskdefs.anymal_terrain_spec(self._loaded_spec, cfg)
        self.anymal_terrain_params = ap = taskdefs.anymal_terrain_params(cfg, spec)
        self.task_params = None
        N = self.num_envs
        self.num_dof = nd = spec.num_dofs
        self.num_bodies = nb = len(spec.bodies)
        self.num_actors = N
        self.max_episode_length = ap.max_episode_length
        self.add_noise = bool(ap.add_noise)
        self.rew_scales = {k: ap.rew_scale[i] for i, k in enumerate(_abi.ANYMAL_TERRAIN_REWARDS)}
        self.rew_scales["termination"] = ap.rew_termination
        sim_cfg = dict(cfg, env=dict(env, plane=ter))   # the ground's friction is env.terrain.staticFriction
        self.sim_params = taskdefs.sim_params(sim_cfg, taskdefs.TASK_INFO["AnymalTerrain"][5], 1)
        dev, f = self.device, torch.float32
        self.dof_names = list(spec.dof_names)
        self.feet_indices = torch.tensor(list(ap.foot_body), device=dev, dtype=torch.long)
        self.knee_indices = torch.tensor(list(ap.knee_body), device=dev, dtype=torch.long)
        self.base_index = int(ap.base_body)
        z = lambda *s, dtype=f: torch.zeros(s, device=dev, dtype=dtype)   # noqa: E731
        # the terrain and where the envs start on it (anymal_terrain.py:257-277)
        gen = torch.Generator().manual_seed(self.seed)
        if not self.curriculum:
            ter["maxInitMapLevel"] = ter["numLevels"] - 1
        self.terrain_levels = torch.randint(0, ter["maxInitMapLevel"] + 1, (N,), generator=gen).to(dev, torch.int32)
        self.terrain_types = torch.randint(0, ter["numTerrains"], (N,), generator=gen).to(dev, torch.int32)
        self.env_origins = z(N, 3)
        self.terrain = Terrain(ter, num_robots=N)
        if self.custom_origins:
            self.terrain_origins = torch.from_numpy(self.terrain.env_origins).to(dev).to(f).contiguous()
            self.env_origins[:] = self.terrain_origins[self.terrain_levels.long(), self.terrain_types.long()]
            self.height_samples = torch.from_numpy(self.terrain.heightsamples).to(dev)
        else:
            self.terrain_origins, self.height_samples = z(1, 1, 3), None
        self.initial_root_states = torch.tensor(self.base_init_state, device=dev, dtype=f).repeat(N, 1).contiguous()
        self.initial_root_states[:, :3] += self.env_origins
        self.root_states = self.initial_root_states.clone()   # world coordinates, as the reference's
        self.dof_state = z(N * nd, 2)
        self.dof_pos = self.dof_state.view(N, nd, 2)[..., 0]
        self.dof_vel = self.dof_state.view(N, nd, 2)[..., 1]
        self.dof_actuation = z(N * nd)
        self.net_contact_force_tensor = z(N * nb, 3)
        self.contact_forces = self.net_contact_force_tensor.view(N, nb, 3)
        self.commands = z(N, 4)   # x vel, y vel, yaw vel, heading
        self.commands_scale = torch.tensor([self.lin_vel_scale, self.lin_vel_scale, self.ang_vel_scale], device=dev)
        self.torques, self.last_actions, self.last_dof_vel = z(N, nd), z(N, nd), z(N, nd)
        self.feet_air_time = z(N, 4)
        self._episode_sums = z(N, _abi.MG_ANYMAL_TERRAIN_REWARDS)
        self.episode_sums = {k: self._episode_sums[:, i] for i, k in enumerate(_abi.ANYMAL_TERRAIN_REWARDS)}
        self._episode_out = z(_abi.MG_ANYMAL_TERRAIN_REWARDS + 1)
        self.measured_heights = z(N, _abi.MG_ANYMAL_TERRAIN_HEIGHT_POINTS)
        self.num_height_points = _abi.MG_ANYMAL_TERRAIN_HEIGHT_POINTS
        pts = torch.from_numpy(taskdefs.anymal_terrain_height_points()).to(dev)
        self.height_points = torch.cat([pts, z(self.num_height_points, 1)], 1).repeat(N, 1, 1)
        self.default_dof_pos = torch.tensor(list(ap.default_dof_pos), device=dev, dtype=f).repeat(N, 1)
        self.gravity_vec = torch.tensor([0.0, 0.0, -1.0], device=dev, dtype=f).repeat(N, 1)
        self.forward_vec = torch.tensor([1.0, 0.0, 0.0], device=dev, dtype=f).repeat(N, 1)
        self.noise_scale_vec = torch.tensor(list(ap.noise_scale_vec), device=dev, dtype=f)
        lo, hi = taskdefs.dof_limits(spec)
        self.dof_limits_lower = torch.tensor(lo, device=dev, dtype=f)
        self.dof_limits_upper = torch.tensor(hi, device=dev, dtype=f)
        self._partials = z((N + 3) // 4, 16)
        self._reset_mark = z(N, dtype=torch.int32)
        v = _abi.StateViews()
        v.root_states, v.dof_state = _abi.ptr(self.root_states), _abi.ptr(self.dof_state)
        v.dof_actuation = _abi.ptr(self.dof_actuation)
        v.net_contact_forces = _abi.ptr(self.net_contact_force_tensor)
        self._create_sim_handle(spec, v)
        if self.custom_origins:
            t = self.terrain
            self.set_heightfield(self.height_samples, t.horizontal_scale, t.vertical_scale,
                                 origin=(-t.border_size, -t.border_size), env_origins=None)
            table = self._heightfield[0]
            ap.hf_heights, ap.hf_nx, ap.hf_ny = table.data_ptr(), table.shape[0], table.shape[1]
            ap.hf_dx, ap.hf_x0, ap.hf_y0 = t.horizontal_scale, -t.border_size, -t.border_size
            ap.env_length, ap.env_rows, ap.env_cols, ap.custom_origins = t.env_length, t.env_rows, t.env_cols, 1
        av = _abi.AnymalTerrainViews()
        av.commands, av.torques = _abi.ptr(self.commands), _abi.ptr(self.torques)
        av.last_actions, av.last_dof_vel = _abi.ptr(self.last_actions), _abi.ptr(self.last_dof_vel)
        av.feet_air_time, av.episode_sums = _abi.ptr(self.feet_air_time), _abi.ptr(self._episode_sums)
        av.terrain_levels, av.terrain_types = _abi.ptr(self.terrain_levels), _abi.ptr(self.terrain_types)
        av.env_origins, av.terrain_origins = _abi.ptr(self.env_origins), _abi.ptr(self.terrain_origins)
        av.dof_actuation, av.episode_out = _abi.ptr(self.dof_actuation), _abi.ptr(self._episode_out)
        av.measured_heights = _abi.ptr(self.measured_heights)
        av.partials, av.reset_mark = _abi.ptr(self._partials), _abi.ptr(self._reset_mark)
        self._bind_task(ap, av, noise_shape=(N, _abi.MG_ANYMAL_TERRAIN_NOISE_COLS))

    # ---------------------------------------------------------------------------------- hot path
    def _launch_step(self, tb, stream):
        lib, sim, p, v, b = self._lib, self.sim, self._params_ref, self._views_ref, _abi.C.byref(tb)
        for _ in range(self.decimation):   # anymal_terrain.py:443-451
            _abi.check(self._pre(sim, p, v, b, stream), lib)
            _abi.check(self._simulate(sim, stream), lib)
        self.common_step_counter += 1      # anymal_terrain.py:460-462
        self._task_views.push_now = int(self.push_robots and self.common_step_counter % self.push_interval == 0)
        _abi.check(self._post(sim, p, v, b, None, stream), lib)

    def post_step_extras(self):
        self._fill_episode()

    def _fill_episode(self):
        """extras["episode"]: views of the device means (the launch that saw a reset rewrote them; no host sync)"""
        ep = self.extras.setdefault("episode", {})
        for i, k in enumerate(_abi.ANYMAL_TERRAIN_REWARDS):
            ep["rew_" + k] = self._episode_out[i]
        ep["terrain_level"] = self._episode_out[_abi.MG_ANYMAL_TERRAIN_REWARDS]

    # ---------------------------------------------------------------------------------- API
    def reset_idx(self, env_ids, goal_env_ids=None, update_levels=True):
        """reset_idx(ids) (anymal_terrain.py:384-425), applied now on the listed ids; ``update_levels=False`` is the
        constructor's reset, which leaves the terrain levels alone"""
        ids = torch.as_tensor(env_ids, device=self.device).flatten().to(torch.int32).contiguous()
        if ids.numel() == 0:
            return
        self._reset_ids = ids   # alive until the launch has consumed it
        tb = self._tb
        tb.step_counter = self.control_steps
        tb.noise = _abi.ptr(self._reset_noise(int(ids.numel())))
        _abi.check(self._reset(self.sim, self._params_ref, self._views_ref, _abi.C.byref(tb), ids.data_ptr(),
                               int(ids.numel()), int(bool(update_levels)), self._stream()), self._lib)
        self._fill_episode()

    def get_heights(self, env_ids=None):
        """the terrain heights under the 140 points around each base, from the current root states (mg_height_scan)"""
        if not self.custom_origins:
            return torch.zeros((self.num_envs, self.num_height_points), device=self.device)
        h = self.height_scan(self.height_points[0, :, :2].contiguous())
        return h if env_ids is None else h[env_ids]

    env_state_tensors = state_tensors(drop=("sensor_tensor", "dof_force_tensor"),
                                      add=("net_contact_force_tensor", "commands", "torques", "last_actions",
                                           "last_dof_vel", "feet_air_time", "_episode_sums", "_episode_out",
                                           "terrain_levels", "terrain_types", "env_origins", "measured_heights"))
    env_state_scalars = SimulateTask.env_state_scalars + ("common_step_counter",)
