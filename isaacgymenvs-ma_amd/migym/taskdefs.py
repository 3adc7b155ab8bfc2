"""Per-task constants -> ``mg_task_params`` / ``mg_sim_params``.

What the reference task constructors compute once at setup
(tasks/ant.py:43-114 + 135-212, tasks/humanoid.py:43-117 + 138-217,
tasks/cartpole.py:36-113, tasks/shadow_hand.py:40-400) and then pass to their jit
functions every step.
"""
from __future__ import annotations

import math

import numpy as np

from . import _abi
from . import model as M

TASK_INFO = {
    # name: (task_id, model table, num_obs, num_actions, start z, max_contacts)
    "Cartpole": (_abi.MG_TASK_CARTPOLE, "cartpole", 4, 1, 2.0, 4),
    "Ant": (_abi.MG_TASK_ANT, "ant", 60, 8, 0.44, 16),
    "Humanoid": (_abi.MG_TASK_HUMANOID, "humanoid", 108, 21, 1.34, 32),
    "ShadowHand": (_abi.MG_TASK_SHADOW_HAND, "shadow_hand", 211, 20, 0.5, 24),
}
# observationType -> (layout id, obs size) (shadow_hand.py:108-113; layouts in csrc/hand_task.hpp)
HAND_OBS = {"full_state": (0, 211), "full": (1, 157), "full_no_vel": (2, 77), "openai": (3, 42)}
TASK_INFO["MAAnt"] = TASK_INFO["Ant"]   # per-agent physics/obs of the multi-agent Ant are the Ant's
# FrankaReachMA has no fused-kernel task id and no shipped table (env.asset.modelTable names one); its obs size depends
# on numAgents / numTargets (reach_params); z = franka_start_z (franka_reach_MA.py:415)
TASK_INFO["FrankaReachMA"] = (None, None, 0, 6, 1.0 + 0.05 / 2 + 0.1, 8)
# Anymal: no fused-kernel task id and no shipped table either; z = baseInitState.pos[2]; 48 contacts put the 13-node
# model on the (32, 32, 48, 48, 192) instance (37 geoms need MG >= 48 anyway)
TASK_INFO["Anymal"] = (None, None, 48, 12, 0.62, 48)

# VecTask.render / render_envs: the default frame and camera of each task (migym/render.py).  eye / target are offsets
# from the root position of the env's actor 0 (follow) or from the env origin; cfg["env"]["render"] overrides any key.
RENDER_DEFAULTS = {
    "Cartpole": dict(width=320, height=240, fov_deg=60.0, eye=(4.0, 0.0, 0.5), target=(0.0, 0.0, 0.0), follow=True),
    "Ant": dict(width=320, height=240, fov_deg=60.0, eye=(2.5, -2.5, 1.5), target=(0.0, 0.0, 0.0), follow=True),
    "Humanoid": dict(width=320, height=240, fov_deg=60.0, eye=(2.2, -2.2, 0.8), target=(0.0, 0.0, -0.2), follow=True),
    "ShadowHand": dict(width=320, height=240, fov_deg=60.0, eye=(0.45, -0.85, 0.45), target=(0.0, -0.3, 0.1),
                       follow=True),
    "MAAnt": dict(width=320, height=240, fov_deg=60.0, eye=(4.0, -4.0, 3.0), target=(0.0, 0.0, 0.0), follow=False),
    "FrankaReachMA": dict(width=320, height=240, fov_deg=60.0, eye=(1.2, -1.2, 1.9), target=(0.0, 0.0, 1.15),
                          follow=False),
    "Anymal": dict(width=320, height=240, fov_deg=60.0, eye=(1.6, -1.6, 0.9), target=(0.0, 0.0, -0.1), follow=True),
}


def render_settings(task: str, cfg: dict) -> dict:
    """RENDER_DEFAULTS[task] with the overrides of cfg["env"]["render"] (width, height, fov_deg, eye, target, follow)"""
    d = dict(RENDER_DEFAULTS.get(task, RENDER_DEFAULTS["Ant"]))
    over = dict((cfg.get("env", {}) or {}).get("render", {}) or {})
    unknown = set(over) - set(d)
    if unknown:
        raise ValueError(f"env.render: unknown keys {sorted(unknown)} (known: {sorted(d)})")
    d.update(over)
    return d


# build-defined solver constants
BAUMGARTE = 0.2
LIMIT_MARGIN = 0.1


def sim_params(cfg: dict, max_contacts: int, agents: int = 1) -> _abi.SimParams:
    s = cfg["sim"]
    px = s.get("physx", {})
    p = _abi.SimParams()
    p.dt = float(s["dt"])
    p.substeps = int(s.get("substeps", 2))
    for i, g in enumerate(s.get("gravity", [0.0, 0.0, -9.81])):
        p.gravity[i] = float(g)
    p.pos_iters = int(px.get("num_position_iterations", 4))
    p.contact_offset = float(px.get("contact_offset", 0.02))
    p.rest_offset = float(px.get("rest_offset", 0.0))
    p.max_depen_vel = float(px.get("max_depenetration_velocity", 10.0))
    plane = cfg["env"].get("plane", {})
    p.friction = float(plane.get("staticFriction", 1.0))
    p.baumgarte = BAUMGARTE
    p.limit_margin = LIMIT_MARGIN
    p.max_contacts = int(max_contacts)
    p.agents = int(agents)
    # the solver: north_star fixes PGS for this build, so the reference's `physx.solver_type` (config.yaml:31, 1 = TGS
    # by default) does not select it; `physx.solver: tgs` opts in to the build's TGS
    solver = str(px.get("solver", "pgs")).lower()
    if solver not in ("pgs", "tgs"):
        raise ValueError(f"sim.physx.solver must be 'pgs' or 'tgs', got {solver!r}")
    p.solver_type = _abi.MG_SOLVER_TGS if solver == "tgs" else _abi.MG_SOLVER_PGS
    p.vel_iters = int(px.get("num_velocity_iterations", 0))
    return p


def dof_limits(spec: M.ModelSpec):
    """lower/upper as the reference reads them (swapped when lower > upper: ant.py:199-206)."""
    lo, hi = [], []
    for n in spec.nodes[1:]:
        a, b = n.lower, n.upper
        if a > b:
            a, b = b, a
        lo.append(a)
        hi.append(b)
    return lo, hi


def agent_offsets(A: int, spacing: float):
    """Agent k of an env starts at (col, row) of a ceil(sqrt(A))-wide grid, centred on the env origin."""
    cols = int(math.ceil(math.sqrt(A)))
    rows = int(math.ceil(A / cols))
    out = []
    for k in range(A):
        c, r = k % cols, k // cols
        out.append(((c - (cols - 1) / 2.0) * spacing, (r - (rows - 1) / 2.0) * spacing, 0.0))
    return out


def hand_spec(object_type: str = "block") -> M.ModelSpec:
    """The ShadowHand model table with the free object of ``objectType`` (shadow_hand.py:86-100, 229-232)."""
    spec = M.load_builtin("shadow_hand")
    spec.obj = M.hand_object(object_type)
    return spec


def hand_task_params(cfg: dict, spec: M.ModelSpec) -> _abi.TaskParams:
    """ShadowHand constants (shadow_hand.py:46-118, 220-330)."""
    env = cfg["env"]
    obs_type = env.get("observationType", "full_state")
    if obs_type not in HAND_OBS:
        raise ValueError(f"Unknown type of observations! observationType should be one of: {sorted(HAND_OBS)}")
    object_type = env.get("objectType", "block")
    if object_type not in ("block", "egg", "pen"):   # shadow_hand.py:86-87
        raise ValueError(f"objectType must be one of block, egg, pen, got {object_type!r}")
    if spec.obj is None or spec.obj["type"] != M.hand_object(object_type)["type"]:
        raise ValueError(f"model's object does not match objectType {object_type!r} (use taskdefs.hand_spec)")
    tp = _abi.TaskParams()
    tp.task_id = _abi.MG_TASK_SHADOW_HAND
    tp.num_agents = 1
    tp.control_freq_inv = max(1, int(env.get("controlFrequencyInv", 1)))   # vec_task.py:381-384
    tp.obs_type, tp.num_obs = HAND_OBS[obs_type]
    tp.num_actions = len(spec.actuators)
    tp.dt = float(cfg["sim"]["dt"])
    tp.clip_actions = float(env.get("clipActions", math.inf))
    tp.clip_obs = float(env.get("clipObservations", math.inf))
    tp.max_episode_length = int(env["episodeLength"])
    if env.get("resetTime", -1.0) > 0.0:   # shadow_hand.py:127-131
        tp.max_episode_length = int(round(env["resetTime"] / (env.get("controlFrequencyInv", 1) * tp.dt)))
    nd = spec.num_dofs
    for j, n in enumerate(spec.nodes[1:]):
        tp.dof_lower[j], tp.dof_upper[j], tp.initial_dof_pos[j] = n.lower, n.upper, 0.0
    for i, a in enumerate(spec.actuators):
        tp.actuated_dof[i] = spec.dof_index(a["joint"])
    tp.rb_per_env = len(spec.bodies) + 2
    tp.num_dofs = spec.num_dofs
    tp.num_fingertips = len(spec.sensors)
    for i, b in enumerate(spec.sensors):
        tp.fingertip_body[i] = b
    tp.max_consecutive_successes = int(env.get("maxConsecutiveSuccesses", 0))
    tp.use_relative_control = int(bool(env.get("useRelativeControl", False)))
    tp.ignore_z_rot = int(object_type == "pen")   # shadow_hand.py:89, 421; also selects randomize_rotation_pen
    tp.dof_speed_scale = float(env["dofSpeedScale"])
    tp.act_moving_average = float(env["actionsMovingAverage"])
    tp.dist_reward_scale = float(env["distRewardScale"])
    tp.rot_reward_scale = float(env["rotRewardScale"])
    tp.rot_eps = float(env["rotEps"])
    tp.action_penalty_scale = float(env["actionPenaltyScale"])
    tp.success_tolerance = float(env["successTolerance"])
    tp.reach_goal_bonus = float(env["reachGoalBonus"])
    tp.fall_dist = float(env["fallDistance"])
    tp.fall_penalty = float(env["fallPenalty"])
    tp.av_factor = float(env.get("averFactor", 0.1))
    tp.vel_obs_scale = 0.2
    tp.force_torque_obs_scale = 10.0
    tp.reset_position_noise = float(env["resetPositionNoise"])
    tp.reset_dof_pos_noise = float(env["resetDofPosRandomInterval"])
    tp.reset_dof_vel_noise = float(env["resetDofVelRandomInterval"])
    # hand at (0, 0, 0.5); object at hand + (0, -0.39, 0.10); goal = object - 0.04 z, drawn displaced
    tp.start_pos[:] = (0.0, 0.0, 0.5)
    tp.start_rot[:] = (0.0, 0.0, 0.0, 1.0)
    tp.object_start[:] = (0.0, 0.0 + -0.39, 0.5 + (0.02 if object_type == "pen" else 0.10))  # :315-318
    tp.goal_displacement[:] = (-0.2, -0.06, 0.12)
    tp.goal_dz = -0.04
    # asymmetric actor-critic: states_buf (N, 211) = compute_full_state(asymm_obs=True) (shadow_hand.py:125-131)
    tp.num_states = 211 if env.get("asymmetric_observations", False) else 0
    # random object forces (shadow_hand.py:69-72, 196-199, 700-706); the per-step decay factor is
    # torch.pow(float32 forceDecay, dt / forceDecayInterval) exactly as the reference evaluates it
    import torch
    tp.object_rb = len(spec.bodies)
    tp.object_rb_mass = float(spec.obj["mass"]) if spec.obj else 0.0
    tp.force_scale = float(env.get("forceScale", 0.0))
    lo, hi = env.get("forceProbRange", [0.001, 0.1])
    tp.force_prob_lo, tp.force_prob_hi = float(lo), float(hi)
    decay = torch.tensor(float(env.get("forceDecay", 0.99)), dtype=torch.float32)
    dt32 = float(torch.tensor(float(cfg["sim"]["dt"]), dtype=torch.float32))  # gymapi.SimParams.dt is a C float
    tp.force_decay_step = float(torch.pow(decay, dt32 / float(env.get("forceDecayInterval", 0.08))))
    del nd
    return tp


def task_params(task: str, cfg: dict, spec: M.ModelSpec) -> _abi.TaskParams:
    if task == "ShadowHand":
        return hand_task_params(cfg, spec)
    base = "Ant" if task == "MAAnt" else task
    task_id, _, nobs, nact, z0, _ = TASK_INFO[base]
    env = cfg["env"]
    tp = _abi.TaskParams()
    tp.task_id = task_id
    tp.num_agents = 1
    tp.control_freq_inv = max(1, int(env.get("controlFrequencyInv", 1)))   # vec_task.py:381-384
    if task == "MAAnt":
        # build-defined multi-agent Ant (SURVEY.md §8(a) A-MA): A ants on a square grid,
        # obs = Ant obs + the other agents' torso positions relative to self (3 (A-1))
        A = int(env.get("numAgents", 4))
        if A < 1 or A > 8 or 64 % A:
            raise ValueError("numAgents must be 1, 2, 4 or 8")
        tp.num_agents = A
        nobs = nobs + 3 * (A - 1)
        for k, off in enumerate(agent_offsets(A, float(env.get("agentSpacing", 2.0)))):
            tp.agent_offset[k][:] = off
    tp.num_obs = nobs
    tp.num_actions = nact
    tp.dt = float(cfg["sim"]["dt"])
    tp.clip_actions = float(env.get("clipActions", math.inf))
    tp.clip_obs = float(env.get("clipObservations", math.inf))
    tp.target[:] = (1000.0, 0.0, 0.0)
    tp.start_pos[:] = (0.0, 0.0, z0)
    tp.start_rot[:] = (0.0, 0.0, 0.0, 1.0)
    if base == "Cartpole":
        tp.max_episode_length = 500                       # cartpole.py:44 (hard-coded)
        tp.power_scale = float(env["maxEffort"])
        tp.reset_dist = float(env["resetDist"])
        return tp
    tp.max_episode_length = int(env["episodeLength"])
    tp.power_scale = float(env["powerScale"])
    tp.dof_vel_scale = float(env["dofVelocityScale"])
    tp.angular_velocity_scale = float(env.get("angularVelocityScale", 0.1))
    tp.contact_force_scale = float(env["contactForceScale"])
    tp.heading_weight = float(env["headingWeight"])
    tp.up_weight = float(env["upWeight"])
    tp.actions_cost_scale = float(env["actionsCost"])
    tp.energy_cost_scale = float(env["energyCost"])
    tp.joints_at_limit_cost_scale = float(env["jointsAtLimitCost"])
    tp.death_cost = float(env["deathCost"])
    tp.termination_height = float(env["terminationHeight"])
    # actuator gears in MJCF actuator order, applied by DOF position (ant.py:159-161, humanoid.py:160-161)
    gears = [a["gear"] for a in spec.actuators]
    for i, g in enumerate(gears):
        tp.motor_effort[i] = float(g)
    tp.max_motor_effort = float(max(gears)) if gears else 1.0
    lo, hi = dof_limits(spec)
    for i, (a, b) in enumerate(zip(lo, hi)):
        tp.dof_lower[i] = a
        tp.dof_upper[i] = b
        # initial_dof_pos: 0 clamped into the limits (ant.py:96-99)
        tp.initial_dof_pos[i] = a if a > 0 else (b if b < 0 else 0.0)
    return tp


# ---- FrankaReachMA (franka_reach_MA.py)
FRANKA_DEFAULT_DOF_POS = [0, 0.1963, 0, -2.6180, 0, 2.9416, 0.7854, 0.035, 0.035]   # franka_reach_MA.py:206-208
FRANKA_CMD_LIMIT = [0.1, 0.1, 0.1, 0.5, 0.5, 0.5]                                  # franka_reach_MA.py:219
REACH_HAND, REACH_EEF = "panda_hand", "panda_grip_site"
REACH_TABLE_THICKNESS, REACH_STAND_HEIGHT, REACH_CUBE_SIZE = 0.05, 0.1, 0.050       # franka_reach_MA.py:270-282


def reach_counts(env: dict):
    """(numAgents, numTargets) as the reference resolves them (franka_reach_MA.py:69-72), validated"""
    A = int(env.get("numAgents", 1))
    T = int(env.get("numTargets", -1))
    if T <= -1:
        T = A
    if A < 1 or A > 8:
        raise ValueError(f"numAgents must be 1..8, got {A}")
    if T < 1 or T > A:
        # the reference's mask[env_ids, nc] indexes an A-wide mask by cube id (franka_reach_MA.py:945-948)
        raise ValueError(f"numTargets must be 1..numAgents ({A}) or -1, got {T}")
    return A, T


def franka_start_poses(A: int, r: float = 0.45):
    """_get_franka_start_poses_rots (franka_reach_MA.py:912-918): base positions (A, 2) on a circle of radius r and
    the rotations about z (A, 4), as float32 tensors"""
    import torch
    rads = torch.deg2rad(torch.tensor(range(0, 359, 360 // A), dtype=torch.float))
    pos = torch.stack([-torch.cos(rads), torch.sin(rads)], dim=-1) * r
    zero = torch.zeros(rads.shape[-1])
    rot = torch.stack([zero, zero, torch.sin(-rads / 2), torch.cos(-rads / 2)], dim=-1)
    return pos[:A], rot[:A]


def reach_spec(spec: M.ModelSpec) -> M.ModelSpec:
    """The arm as the task configures it, on a copy (franka_reach_MA.py:259, 265-266, 309-327): arm joints in effort
    mode (no stiffness, damping or drive), fingers position-driven (kp 5000, damping 100, effort 200), no gravity."""
    import copy
    spec = copy.deepcopy(spec)
    if spec.num_dofs != 9 or not spec.fixed_base:
        raise ValueError("FrankaReachMA needs a fixed-base 9-DOF Franka model (7 arm joints, 2 fingers)")
    for j, n in enumerate(spec.nodes[1:]):
        n.stiffness = 0.0
        if j < 7:
            n.damping, n.drive_kp = 0.0, 0.0
        else:
            n.damping, n.drive_kp, n.effort_limit = 100.0, 5000.0, 200.0
    spec.gravity_off = 1
    return spec


def reach_params(cfg: dict, spec: M.ModelSpec) -> _abi.ReachParams:
    """FrankaReachMA constants (franka_reach_MA.py:40-80, 205-220, 616-704), computed the way the reference's
    expressions do: Python floats where it has floats, a float32 tensor where it has one.  ``spec``: the loaded
    table (its effort limits are the asset's, read before the task raises the fingers' to 200)."""
    import torch
    env = cfg["env"]
    A, T = reach_counts(env)
    rp = _abi.ReachParams()
    rp.num_agents, rp.num_targets = A, T
    rp.num_obs = 10 + 3 * T + 3 * (A - 1)
    rp.max_episode_length = int(env["episodeLength"])
    rp.clip_actions = float(env.get("clipActions", math.inf))
    rp.clip_obs = float(env.get("clipObservations", math.inf))
    rp.action_scale = float(env.get("actionScale", 1.0))
    kp = torch.tensor([150.0] * 6)
    kd = 2 * torch.sqrt(kp)
    kpn = torch.tensor([10.0] * 7)
    kdn = 2 * torch.sqrt(kpn)
    for k in range(6):
        rp.cmd_limit[k] = FRANKA_CMD_LIMIT[k]
        rp.kp[k], rp.kd[k] = float(kp[k]), float(kd[k])
    for k in range(7):
        rp.kp_null[k], rp.kd_null[k] = float(kpn[k]), float(kdn[k])
        rp.osc_default_dof_pos[k] = FRANKA_DEFAULT_DOF_POS[k]
        rp.effort_limit[k] = spec.nodes[1 + k].effort_limit
    rp.jac_body = rp.hand_body = spec.body_index(REACH_HAND)
    rp.eef_body = spec.body_index(REACH_EEF)
    rp.num_bodies, rp.num_dofs = len(spec.bodies), spec.num_dofs
    for j, n in enumerate(spec.nodes[1:10]):
        rp.default_dof_pos[j] = FRANKA_DEFAULT_DOF_POS[j]
        rp.dof_lower[j], rp.dof_upper[j] = n.lower, n.upper
    rp.dof_noise_scale = float(env.get("frankaDofNoise", 0.0)) * 2.0          # franka_reach_MA.py:633
    rp.cube_xy_center[0] = rp.cube_xy_center[1] = 0.0                          # _table_surface_pos[:2]
    rp.cube_xy_scale = 2.0 * float(env.get("startPositionNoise", 0.0))         # franka_reach_MA.py:696
    table_z = 1.0 + REACH_TABLE_THICKNESS / 2                                  # _table_surface_pos[2] (float64)
    cube_heights = torch.ones(1) * REACH_CUBE_SIZE                             # states["cubeA_size"] (float32)
    rp.cube_z_base = float(table_z + cube_heights / 2)                         # franka_reach_MA.py:693
    rp.cube_z_range = 0.5
    return rp


# ---- Quadcopter (quadcopter.py): no fused-kernel task id and no table (M.quadcopter_model builds the model);
# z = the default pose (quadcopter.py:236-237); 16 contacts: the (16, 9, 16, 16, 0) instance
QUADCOPTER_MAX_CONTACTS = 16
TASK_INFO["Quadcopter"] = (None, None, 21, 12, 1.0, QUADCOPTER_MAX_CONTACTS)
RENDER_DEFAULTS["Quadcopter"] = dict(width=320, height=240, fov_deg=60.0, eye=(0.8, -0.8, 0.5), target=(0.0, 0.0, 0.0),
                                     follow=True)
QUADCOPTER_ROTOR_BODIES = (2, 4, 6, 8)   # quadcopter.py:193: the rows of the force tensor that carry the thrusts


def quadcopter_spec(spec: M.ModelSpec = None) -> M.ModelSpec:
    """The quadcopter as the reference's task configures it, on a copy (quadcopter.py:216-221, 239-246): every DOF on a
    position drive of stiffness 1000 and damping 0 without an effort limit, no link angular damping, hinge rates
    capped at 4 pi.  ``spec``: M.quadcopter_model() by default."""
    import copy
    spec = copy.deepcopy(spec) if spec is not None else M.quadcopter_model()
    for n in spec.nodes[1:]:
        n.stiffness, n.damping = 0.0, 0.0
        n.drive_kp, n.effort_limit = 1000.0, float(np.finfo(np.float32).max)
    spec.angular_damping = 0.0
    spec.max_angular_velocity = 4.0 * math.pi
    return spec


def quadcopter_params(cfg: dict, spec: M.ModelSpec) -> _abi.QuadcopterParams:
    """Quadcopter constants (quadcopter.py:43-89, 225-237, 310-315), computed where the reference computes them: the
    two action speed scales times dt as products of Python floats in double, dt the C float gymapi.SimParams.dt is,
    rounded to fp32 once (a Python float times a float tensor)."""
    env = cfg["env"]
    if spec.num_dofs != _abi.MG_QUAD_DOFS or len(spec.bodies) != _abi.MG_QUAD_BODIES or spec.fixed_base:
        raise ValueError("Quadcopter needs the free-base 8-DOF, 9-body model (M.quadcopter_model)")
    qp = _abi.QuadcopterParams()
    dt = float(np.float32(cfg["sim"]["dt"]))
    qp.dof_step, qp.thrust_step = dt * (8 * math.pi), dt * 200
    lo, hi = dof_limits(spec)
    for j in range(_abi.MG_QUAD_DOFS):
        qp.dof_lower[j], qp.dof_upper[j] = lo[j], hi[j]
    qp.thrust_lower, qp.thrust_upper = 0.0, 2.0
    for c, x in enumerate([0.0, 0.0, TASK_INFO["Quadcopter"][4], 0.0, 0.0, 0.0, 1.0] + [0.0] * 6):
        qp.init_root[c] = x
    qp.clip_actions = float(env.get("clipActions", math.inf))
    qp.clip_obs = float(env.get("clipObservations", math.inf))
    qp.max_episode_length = int(env["maxEpisodeLength"])
    for k, b in enumerate(QUADCOPTER_ROTOR_BODIES):
        qp.rotor_body[k] = b
    return qp


# ---- Anymal (anymal.py)
ANYMAL_BASE, ANYMAL_KNEE, ANYMAL_FOOT = "base", "THIGH", "SHANK"   # anymal.py:192-197, 224 (collapsed fixed joints)


def anymal_spec(spec: M.ModelSpec, cfg: dict) -> M.ModelSpec:
    """The quadruped as the task configures it, on a copy (anymal.py:170-180, 199-203): every DOF on a position drive
    with env.control's stiffness and damping (the effort limits stay the asset's), no link angular damping."""
    import copy
    spec = copy.deepcopy(spec)
    if spec.num_dofs != _abi.MG_ANYMAL_DOFS or spec.fixed_base:
        raise ValueError("Anymal needs a free-base 12-DOF model")
    ctl = cfg["env"]["control"]
    for n in spec.nodes[1:]:
        n.stiffness = 0.0
        n.drive_kp, n.damping = float(ctl["stiffness"]), float(ctl["damping"])
    spec.angular_damping = 0.0
    return spec


def anymal_params(cfg: dict, spec: M.ModelSpec) -> _abi.AnymalParams:
    """Anymal constants (anymal.py:46-100, 132-143, 192-224), computed where the reference computes them: products and
    differences of Python floats in double, then rounded to fp32 once."""
    env = cfg["env"]
    learn, ctl = env["learn"], env["control"]
    import numpy as np
    dt = float(np.float32(cfg["sim"]["dt"]))   # self.dt = self.sim_params.dt: gymapi.SimParams.dt is a C float
    ap = _abi.AnymalParams()
    ap.lin_vel_scale, ap.ang_vel_scale = float(learn["linearVelocityScale"]), float(learn["angularVelocityScale"])
    ap.dof_pos_scale, ap.dof_vel_scale = float(learn["dofPositionScale"]), float(learn["dofVelocityScale"])
    ap.action_scale = float(ctl["actionScale"])
    ap.rew_lin_vel_xy = float(learn["linearVelocityXYRewardScale"]) * dt      # anymal.py:99-100
    ap.rew_ang_vel_z = float(learn["angularVelocityZRewardScale"]) * dt
    ap.rew_torque = float(learn["torqueRewardScale"]) * dt
    angles = env["defaultJointAngles"]
    for j, name in enumerate(spec.dof_names):
        ap.default_dof_pos[j] = float(angles[name])
    b = env["baseInitState"]
    state = list(b["pos"]) + list(b["rot"]) + list(b["vLinear"]) + list(b["vAngular"])
    if len(state) != 13:
        raise ValueError("baseInitState must hold pos 3, rot 4, vLinear 3, vAngular 3")
    for c, x in enumerate(state):
        ap.base_init_state[c] = float(x)
    rng = env["randomCommandVelocityRanges"]
    for c, key in enumerate(("linear_x", "linear_y", "yaw")):
        lo, hi = float(rng[key][0]), float(rng[key][1])
        ap.command_lo[c], ap.command_span[c] = lo, hi - lo
    names = [x.name for x in spec.bodies]
    knees = [i for i, s in enumerate(names) if ANYMAL_KNEE in s]
    if len(knees) != 4 or ANYMAL_BASE not in names:
        raise ValueError("Anymal needs a body named 'base' and four THIGH bodies")
    ap.base_body = names.index(ANYMAL_BASE)
    for k, i in enumerate(knees):
        ap.knee_body[k] = i
    ap.num_bodies = len(spec.bodies)
    ap.clip_actions = float(env.get("clipActions", math.inf))
    ap.clip_obs = float(env.get("clipObservations", math.inf))
    ap.max_episode_length = int(float(learn["episodeLength_s"]) / dt + 0.5)   # anymal.py:95
    return ap


# ---- HumanoidAMP (humanoid_amp.py, amp/humanoid_amp_base.py)
AMP_KEY_BODY_NAMES = ["right_hand", "left_hand", "right_foot", "left_foot"]   # humanoid_amp_base.py:47
AMP_DOF_OFFSETS = [0, 3, 6, 9, 10, 13, 14, 17, 18, 21, 24, 25, 28]            # humanoid_amp_base.py:42
# no fused-kernel task id and no shipped table; z = the start pose (humanoid_amp_base.py:209); 48 contacts and the
# model's 34 lanes put it on the (64, 40, 48, 48, 192) instance
TASK_INFO["HumanoidAMP"] = (None, None, _abi.MG_AMP_OBS, _abi.MG_AMP_DOFS, 0.89, 48)
RENDER_DEFAULTS["HumanoidAMP"] = dict(width=320, height=240, fov_deg=60.0, eye=(0.0, -3.0, 0.1),
                                      target=(0.0, 0.0, 0.1), follow=True)   # _init_camera: 3 m along -y


def amp_spec(spec: M.ModelSpec, cfg: dict) -> M.ModelSpec:
    """The AMP humanoid as the task configures it, on a copy (humanoid_amp_base.py:183-187, 237-240).  pdControl:
    every DOF is a position drive whose gains are the MJCF joint's stiffness and damping, which is how gym's DOF
    properties read them (DOF_MODE_POS), and no passive spring remains.  Otherwise DOF_MODE_NONE: efforts only, the
    joint springs passive, as for Humanoid."""
    import copy
    spec = copy.deepcopy(spec)
    if spec.num_dofs != _abi.MG_AMP_DOFS or len(spec.bodies) != _abi.MG_AMP_BODIES or spec.fixed_base:
        raise ValueError("HumanoidAMP needs the free-base AMP humanoid: 28 DOFs, 15 bodies")
    if bool(cfg["env"]["pdControl"]):
        for n in spec.nodes[1:]:
            n.drive_kp, n.stiffness = float(n.stiffness), 0.0
    spec.angular_damping = 0.01          # asset_options.angular_damping
    spec.max_angular_velocity = 100.0    # asset_options.max_angular_velocity
    return spec


def amp_action_offset_scale(spec: M.ModelSpec):
    """_build_pd_action_offset_scale (humanoid_amp_base.py:262-295): 3-DOF joints get +-pi, 1-DOF joints their middle
    +- 0.7 of their range.  The limits are gym's fp32 values; from them on the arithmetic is numpy double, rounded to
    fp32 once at the end (the reference's own intermediate precision depends on the numpy version's scalar promotion;
    the two agree to an fp32 ulp)."""
    import numpy as np
    lo, hi = dof_limits(spec)
    lim_low = np.array(lo, np.float32).astype(np.float64)
    lim_high = np.array(hi, np.float32).astype(np.float64)
    for j in range(len(AMP_DOF_OFFSETS) - 1):
        o, size = AMP_DOF_OFFSETS[j], AMP_DOF_OFFSETS[j + 1] - AMP_DOF_OFFSETS[j]
        if size == 3:
            lim_low[o:o + 3] = -np.pi
            lim_high[o:o + 3] = np.pi
        else:
            curr_low, curr_high = lim_low[o], lim_high[o]
            curr_mid = 0.5 * (curr_high + curr_low)
            curr_scale = 0.7 * (curr_high - curr_low)
            lim_low[o] = curr_mid - curr_scale
            lim_high[o] = curr_mid + curr_scale
    offset = 0.5 * (lim_high + lim_low)
    scale = 0.5 * (lim_high - lim_low)
    return np.asarray(offset, np.float32), np.asarray(scale, np.float32)


def amp_params(cfg: dict, spec: M.ModelSpec) -> _abi.AmpParams:
    """HumanoidAMP constants (humanoid_amp_base.py:54-76, 105-109, 189-258; humanoid_amp.py:60-64)."""
    env = cfg["env"]
    ap = _abi.AmpParams()
    offset, scale = amp_action_offset_scale(spec)
    gears = {a["joint"]: float(a["gear"]) for a in spec.actuators}
    for j, name in enumerate(spec.dof_names):
        ap.pd_action_offset[j], ap.pd_action_scale[j] = float(offset[j]), float(scale[j])
        ap.motor_effort[j] = gears.get(name, 0.0)
        ap.initial_dof_pos[j] = 0.0
    ap.initial_dof_pos[spec.dof_names.index("right_shoulder_x")] = 0.5 * math.pi
    ap.initial_dof_pos[spec.dof_names.index("left_shoulder_x")] = -0.5 * math.pi
    root = [0.0, 0.0, 0.89, 0.0, 0.0, 0.0, 1.0] + [0.0] * 6
    for c, x in enumerate(root):
        ap.initial_root[c] = x
    ap.dt = max(1, int(env.get("controlFrequencyInv", 1))) * float(cfg["sim"]["dt"])   # a Python double, not a C float
    ap.power_scale = float(env["powerScale"])
    ap.termination_height = float(env["terminationHeight"])
    ap.hybrid_init_prob = float(env["hybridInitProb"])
    ap.clip_actions = float(env.get("clipActions", math.inf))
    ap.clip_obs = float(env.get("clipObservations", math.inf))
    ap.max_episode_length = int(env["episodeLength"])
    ap.enable_early_termination = int(bool(env["enableEarlyTermination"]))
    ap.local_root_obs = int(bool(env["localRootObs"]))
    ap.pd_control = int(bool(env["pdControl"]))
    if env["stateInit"] not in _abi.MG_AMP_INIT:
        raise ValueError(f"stateInit must be one of {sorted(_abi.MG_AMP_INIT)}, got {env['stateInit']!r}")
    ap.state_init = _abi.MG_AMP_INIT[env["stateInit"]]
    steps = int(env["numAMPObsSteps"])
    if not 2 <= steps <= _abi.MG_AMP_MAX_OBS_STEPS:
        raise ValueError(f"numAMPObsSteps must be 2 .. {_abi.MG_AMP_MAX_OBS_STEPS}, got {steps}")
    ap.num_amp_obs_steps = steps
    names = [b.name for b in spec.bodies]
    for k, name in enumerate(AMP_KEY_BODY_NAMES):
        ap.key_body[k] = names.index(name)
    mask = 0
    for name in env["contactBodies"]:
        mask |= 1 << names.index(name)
    ap.contact_body_mask = mask
    ap.num_bodies = len(names)
    return ap


# ---- AnymalTerrain (anymal_terrain.py)
# as Anymal: no fused-kernel task id, no shipped table, z = baseInitState.pos[2], the (32, 32, 48, 48, 192) instance
TASK_INFO["AnymalTerrain"] = (None, None, _abi.MG_ANYMAL_TERRAIN_OBS, _abi.MG_ANYMAL_DOFS, 0.62, 48)
RENDER_DEFAULTS["AnymalTerrain"] = dict(RENDER_DEFAULTS["Anymal"])
ANYMAL_TERRAIN_HIP_DOFS = (0, 3, 6, 9)   # anymal_terrain.py:359
# the learn.* key of each column of rew_scale / episode_sums (_abi.ANYMAL_TERRAIN_REWARDS; anymal_terrain.py:63-76)
ANYMAL_TERRAIN_REWARD_KEYS = (
    "linearVelocityXYRewardScale", "linearVelocityZRewardScale", "angularVelocityZRewardScale",
    "angularVelocityXYRewardScale", "orientationRewardScale", "torqueRewardScale", "jointAccRewardScale",
    "baseHeightRewardScale", "feetAirTimeRewardScale", "kneeCollisionRewardScale", "feetStumbleRewardScale",
    "actionRateRewardScale", "hipRewardScale")


def anymal_terrain_spec(spec: M.ModelSpec, cfg: dict) -> M.ModelSpec:
    """The quadruped as the task configures it, on a copy (anymal_terrain.py:218-231): DOF_MODE_EFFORT, so no drive
    gain and no joint spring; the joint damping and the effort limits stay the asset's; no link angular damping."""
    import copy
    spec = copy.deepcopy(spec)
    if spec.num_dofs != _abi.MG_ANYMAL_DOFS or spec.fixed_base:
        raise ValueError("AnymalTerrain needs a free-base 12-DOF model")
    for n in spec.nodes[1:]:
        n.stiffness = 0.0
        n.drive_kp = 0.0
    spec.angular_damping = 0.0
    return spec


def anymal_terrain_height_points():
    """init_height_points (anymal_terrain.py:503-513): the (140, 2) grid of the 1 m x 1.6 m rectangle without its
    centre lines, x major, each coordinate the fp32 product 0.1 * k as torch forms it"""
    y = np.float32(0.1) * np.array([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5], np.float32)
    x = np.float32(0.1) * np.array([-8, -7, -6, -5, -4, -3, -2, 2, 3, 4, 5, 6, 7, 8], np.float32)
    gx, gy = np.meshgrid(x, y, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)


def anymal_terrain_noise_scale_vec(cfg: dict):
    """_get_noise_scale_vec (anymal_terrain.py:174-186): each entry a product of Python floats, rounded to fp32 once"""
    learn = cfg["env"]["learn"]
    level = learn["noiseLevel"]
    v = np.zeros(_abi.MG_ANYMAL_TERRAIN_OBS, np.float32)
    v[0:3] = learn["linearVelocityNoise"] * level * learn["linearVelocityScale"]
    v[3:6] = learn["angularVelocityNoise"] * level * learn["angularVelocityScale"]
    v[6:9] = learn["gravityNoise"] * level
    v[12:24] = learn["dofPositionNoise"] * level * learn["dofPositionScale"]
    v[24:36] = learn["dofVelocityNoise"] * level * learn["dofVelocityScale"]
    v[36:176] = learn["heightMeasurementNoise"] * level * learn["heightMeasurementScale"]
    return v


def anymal_terrain_params(cfg: dict, spec: M.ModelSpec) -> _abi.AnymalTerrainParams:
    """AnymalTerrain constants (anymal_terrain.py:53-105, 174-186, 245-292), computed where the reference computes them:
    products and differences of Python floats in double, rounded to fp32 once.  The terrain fields (env_length,
    env_rows, env_cols, custom_origins, hf_*) are the task's to fill once it has built its Terrain."""
    env = cfg["env"]
    learn, ctl, ter = env["learn"], env["control"], env["terrain"]
    ap = _abi.AnymalTerrainParams()
    ap.lin_vel_scale, ap.ang_vel_scale = float(learn["linearVelocityScale"]), float(learn["angularVelocityScale"])
    ap.dof_pos_scale, ap.dof_vel_scale = float(learn["dofPositionScale"]), float(learn["dofVelocityScale"])
    ap.height_meas_scale = float(learn["heightMeasurementScale"])
    dt = ctl["decimation"] * cfg["sim"]["dt"]   # anymal_terrain.py:95: Python floats
    for k, key in enumerate(ANYMAL_TERRAIN_REWARD_KEYS):
        ap.rew_scale[k] = learn[key] * dt
    ap.rew_termination = learn["terminalReward"] * dt
    # what feet_air_time advances by is self.dt as VecTask.__init__ leaves it (vec_task.py:242 overwrites the task's
    # decimation * dt with sim_params.dt, a C float): the reference's quirk, kept
    ap.dt = float(np.float32(cfg["sim"]["dt"]))
    ap.Kp, ap.Kd, ap.action_scale, ap.torque_clip = float(ctl["stiffness"]), float(ctl["damping"]), \
        float(ctl["actionScale"]), 80.0
    angles = env["defaultJointAngles"]
    for j, name in enumerate(spec.dof_names):
        ap.default_dof_pos[j] = float(angles[name])
    b = env["baseInitState"]
    state = list(b["pos"]) + list(b["rot"]) + list(b["vLinear"]) + list(b["vAngular"])
    if len(state) != 13:
        raise ValueError("baseInitState must hold pos 3, rot 4, vLinear 3, vAngular 3")
    for c, x in enumerate(state):
        ap.base_init_state[c] = float(x)
    rng = env["randomCommandVelocityRanges"]
    for c, key in enumerate(("linear_x", "linear_y", "yaw")):   # the yaw range is the heading's (anymal_terrain.py:411)
        lo, hi = float(rng[key][0]), float(rng[key][1])
        ap.command_lo[c], ap.command_span[c] = lo, hi - lo
    urdf = env.get("urdfAsset", {}) or {}
    foot_name, knee_name = urdf.get("footName", ANYMAL_FOOT), urdf.get("kneeName", ANYMAL_KNEE)
    names = [x.name for x in spec.bodies]
    knees = [i for i, s in enumerate(names) if knee_name in s]
    feet = [i for i, s in enumerate(names) if foot_name in s]
    if len(knees) != 4 or len(feet) != 4 or ANYMAL_BASE not in names:
        raise ValueError(f"AnymalTerrain needs a body named 'base', four {knee_name} and four {foot_name} bodies")
    ap.base_body = names.index(ANYMAL_BASE)
    for k in range(4):
        ap.knee_body[k], ap.foot_body[k], ap.hip_dof[k] = knees[k], feet[k], ANYMAL_TERRAIN_HIP_DOFS[k]
    ap.num_bodies = len(names)
    ap.allow_knee_contacts = int(bool(learn["allowKneeContacts"]))
    ap.add_noise = int(bool(learn["addNoise"]))
    for c, x in enumerate(anymal_terrain_noise_scale_vec(cfg)):
        ap.noise_scale_vec[c] = float(x)
    ap.max_episode_length_s = float(learn["episodeLength_s"])
    ap.max_episode_length = int(learn["episodeLength_s"] / dt + 0.5)
    ap.curriculum = int(bool(ter["curriculum"]))
    ap.env_length, ap.env_rows, ap.env_cols, ap.custom_origins = 0.0, 1, 1, 0
    for k, x in enumerate(anymal_terrain_height_points().ravel()):
        ap.height_points[k] = float(x)
    ap.clip_actions = float(env.get("clipActions", math.inf))
    ap.clip_obs = float(env.get("clipObservations", math.inf))
    return ap
