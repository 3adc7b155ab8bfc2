"""ctypes mirror of ``include/migym.h`` and the loader for ``libmigym.so``.

The product path calls ONLY the HIP library built from ``csrc/`` (see
``build.py``).  If the library is missing, :func:`lib` raises: there is no CPU
fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import model as _model

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "_lib", "libmigym.so")

MG_TASK_CARTPOLE, MG_TASK_ANT, MG_TASK_HUMANOID, MG_TASK_SHADOW_HAND = 0, 1, 2, 3
MG_SET_ROOT_STATE, MG_SET_DOF_STATE, MG_SET_DOF_TARGET = 0, 1, 2
MG_MAX_HAND_DOFS = 32
# [goal-only 4 | reset_idx 53 | reset_target_pose 4 | force-prob redraw 1 | force select 1 | force dir 3]
# (shadow_hand.py:587, 610, 642-643, 704-706)
HAND_NOISE_COLS = 66
MG_ENV_SPACE, MG_LOCAL_SPACE, MG_GLOBAL_SPACE = 0, 1, 2


class SimParams(C.Structure):
    _fields_ = [("dt", C.c_float), ("substeps", C.c_int32), ("gravity", C.c_float * 3),
                ("pos_iters", C.c_int32), ("contact_offset", C.c_float), ("rest_offset", C.c_float),
                ("max_depen_vel", C.c_float), ("friction", C.c_float), ("baumgarte", C.c_float),
                ("limit_margin", C.c_float), ("max_contacts", C.c_int32), ("agents", C.c_int32),
                ("solver_type", C.c_int16), ("vel_iters", C.c_int16)]


MG_SOLVER_PGS, MG_SOLVER_TGS = 0, 1


class StateViews(C.Structure):
    _fields_ = [("root_states", C.c_void_p), ("dof_state", C.c_void_p), ("dof_actuation", C.c_void_p),
                ("sensors", C.c_void_p), ("dof_force", C.c_void_p), ("rigid_body_states", C.c_void_p),
                ("dof_targets", C.c_void_p), ("rb_forces", C.c_void_p), ("rb_force_space", C.c_int32),
                ("env_props_stride", C.c_int32), ("env_props", C.c_void_p), ("net_contact_forces", C.c_void_p)]


# ---- domain randomization (include/migym.h; vec_task.py:612-842, dr_utils.py)
MG_EP_NODE, MG_EP_GEOM, MG_EP_TENDON, MG_EP_OBJECT = 0, 1, 2, 3
MG_EP_NODE_WIDTH = 9   # [mass, armature, damping, stiffness, lower, upper, drive kp, effort, frictionloss]
MG_DR_UNIFORM, MG_DR_GAUSSIAN, MG_DR_LOGUNIFORM = 0, 1, 2
MG_DR_ADDITIVE, MG_DR_SCALING = 0, 1
MG_DR_SCHED_NONE, MG_DR_SCHED_LINEAR, MG_DR_SCHED_CONSTANT = 0, 1, 2


class DrDesc(C.Structure):
    _fields_ = [("distribution", C.c_int32), ("operation", C.c_int32), ("schedule", C.c_int32),
                ("schedule_steps", C.c_int32), ("num_buckets", C.c_int32), ("after_setup", C.c_int32),
                ("range", C.c_float * 2)]


class DrAttr(C.Structure):
    _fields_ = [("slot", C.c_int32), ("desc", C.c_int32), ("og", C.c_float), ("pad", C.c_int32)]


class DrApplyArgs(C.Structure):
    _fields_ = [("descs", C.c_void_p), ("attrs", C.c_void_p), ("nattr", C.c_int32), ("stride", C.c_int32),
                ("n", C.c_int32), ("frequency", C.c_int32), ("first", C.c_int32), ("increment", C.c_int32),
                ("last_step", C.c_int64), ("env_props", C.c_void_p), ("reset_mask", C.c_void_p),
                ("randomize_buf", C.c_void_p), ("samples", C.c_void_p), ("seed", C.c_uint64),
                ("counter", C.c_uint64), ("env_offset", C.c_int64)]


class DrNoiseArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_clamped", C.c_void_p), ("clip", C.c_float), ("distribution", C.c_int32),
                ("operation", C.c_int32), ("refresh_corr", C.c_int32), ("corr", C.c_void_p), ("n", C.c_int64),
                ("scale", C.c_float), ("shift", C.c_float), ("c_scale", C.c_float), ("c_shift", C.c_float),
                ("injected", C.c_void_p), ("injected_corr", C.c_void_p), ("seed", C.c_uint64),
                ("counter", C.c_uint64), ("elem_offset", C.c_int64), ("key", C.c_uint32), ("pad", C.c_int32)]


class TaskParams(C.Structure):
    _fields_ = [("task_id", C.c_int32), ("num_obs", C.c_int32), ("num_actions", C.c_int32),
                ("max_episode_length", C.c_int32), ("dt", C.c_float), ("clip_actions", C.c_float),
                ("clip_obs", C.c_float), ("power_scale", C.c_float), ("dof_vel_scale", C.c_float),
                ("angular_velocity_scale", C.c_float), ("contact_force_scale", C.c_float),
                ("heading_weight", C.c_float), ("up_weight", C.c_float), ("actions_cost_scale", C.c_float),
                ("energy_cost_scale", C.c_float), ("joints_at_limit_cost_scale", C.c_float),
                ("death_cost", C.c_float), ("termination_height", C.c_float), ("max_motor_effort", C.c_float),
                ("reset_dist", C.c_float), ("target", C.c_float * 3), ("start_pos", C.c_float * 3),
                ("start_rot", C.c_float * 4), ("motor_effort", C.c_float * 64), ("dof_lower", C.c_float * 64),
                ("dof_upper", C.c_float * 64), ("initial_dof_pos", C.c_float * 64),
                ("num_agents", C.c_int32), ("control_freq_inv", C.c_int32), ("agent_offset", (C.c_float * 3) * 8),
                # in-hand manipulation (MG_TASK_SHADOW_HAND)
                ("num_fingertips", C.c_int32), ("fingertip_body", C.c_int32 * 8),
                ("actuated_dof", C.c_int32 * MG_MAX_HAND_DOFS), ("max_consecutive_successes", C.c_int32),
                ("use_relative_control", C.c_int32), ("ignore_z_rot", C.c_int32), ("obs_type", C.c_int32),
                ("rb_per_env", C.c_int32), ("num_dofs", C.c_int32),
                ("dof_speed_scale", C.c_float), ("act_moving_average", C.c_float),
                ("dist_reward_scale", C.c_float), ("rot_reward_scale", C.c_float), ("rot_eps", C.c_float),
                ("action_penalty_scale", C.c_float), ("success_tolerance", C.c_float),
                ("reach_goal_bonus", C.c_float), ("fall_dist", C.c_float), ("fall_penalty", C.c_float),
                ("av_factor", C.c_float), ("vel_obs_scale", C.c_float), ("force_torque_obs_scale", C.c_float),
                ("reset_position_noise", C.c_float), ("reset_dof_pos_noise", C.c_float),
                ("reset_dof_vel_noise", C.c_float), ("object_start", C.c_float * 3),
                ("goal_displacement", C.c_float * 3), ("goal_dz", C.c_float),
                ("num_states", C.c_int32), ("object_rb", C.c_int32), ("force_scale", C.c_float),
                ("force_decay_step", C.c_float), ("force_prob_lo", C.c_float), ("force_prob_hi", C.c_float),
                ("object_rb_mass", C.c_float), ("obs_map", C.c_uint16 * 256), ("state_map", C.c_uint16 * 256)]


class TaskBuffers(C.Structure):
    _fields_ = [("actions", C.c_void_p), ("actions_out", C.c_void_p), ("obs", C.c_void_p),
                ("obs_clamped", C.c_void_p), ("rew", C.c_void_p), ("reset", C.c_void_p),
                ("progress", C.c_void_p), ("timeout", C.c_void_p), ("potentials", C.c_void_p),
                ("prev_potentials", C.c_void_p), ("up_vec", C.c_void_p), ("heading_vec", C.c_void_p),
                ("noise", C.c_void_p), ("seed", C.c_uint64), ("step_counter", C.c_uint64),
                ("env_offset", C.c_int64),
                ("prev_targets", C.c_void_p), ("goal_states", C.c_void_p), ("reset_goal", C.c_void_p),
                ("successes", C.c_void_p), ("consecutive_successes", C.c_void_p), ("reduce_scratch", C.c_void_p),
                ("states", C.c_void_p), ("random_force_prob", C.c_void_p), ("out_pack", C.c_void_p),
                ("defer_finalize", C.c_int32), ("pad_tb", C.c_int32)]


class Replay(C.Structure):
    """mg_replay: the post-simulate state mg_env_step_replay injects in place of gym.simulate (tests)."""
    _fields_ = [("root_states", C.c_void_p), ("dof_state", C.c_void_p), ("sensors", C.c_void_p),
                ("dof_force", C.c_void_p), ("rigid_body_states", C.c_void_p), ("pre_root_states", C.c_void_p),
                ("pre_dof_state", C.c_void_p)]


class DynamicsViews(C.Structure):
    """mg_dynamics_views: the Jacobian (N*A, nB-1, 6, nD) and mass-matrix (N*A, nD, nD) tensors."""
    _fields_ = [("jacobian", C.c_void_p), ("mass_matrix", C.c_void_p)]


class OscArgs(C.Structure):
    """mg_osc_args: one operational-space control launch (franka_reach_MA.py:770-802)."""
    _fields_ = [("arm_dofs", C.c_int32), ("jac_body", C.c_int32), ("dpose", C.c_void_p), ("eef_vel", C.c_void_p),
                ("eef_vel_stride", C.c_int64), ("kp", C.c_float * 6), ("kd", C.c_float * 6),
                ("kp_null", C.c_float * 7), ("kd_null", C.c_float * 7), ("default_dof_pos", C.c_float * 7),
                ("effort_limit", C.c_float * 7), ("out", C.c_void_p), ("out_stride", C.c_int64),
                ("out_cols", C.c_int32), ("pad_osc", C.c_int32), ("jac_in", C.c_void_p), ("mm_in", C.c_void_p)]


class ReachParams(C.Structure):
    """mg_reach_params: the constants of FrankaReachMA (taskdefs.reach_params)."""
    _fields_ = [("num_agents", C.c_int32), ("num_targets", C.c_int32), ("num_obs", C.c_int32),
                ("max_episode_length", C.c_int32), ("clip_actions", C.c_float), ("clip_obs", C.c_float),
                ("action_scale", C.c_float), ("cmd_limit", C.c_float * 6), ("kp", C.c_float * 6),
                ("kd", C.c_float * 6), ("kp_null", C.c_float * 7), ("kd_null", C.c_float * 7),
                ("osc_default_dof_pos", C.c_float * 7), ("effort_limit", C.c_float * 7), ("jac_body", C.c_int32),
                ("eef_body", C.c_int32), ("hand_body", C.c_int32), ("num_bodies", C.c_int32),
                ("num_dofs", C.c_int32), ("default_dof_pos", C.c_float * 9), ("dof_lower", C.c_float * 9),
                ("dof_upper", C.c_float * 9), ("dof_noise_scale", C.c_float), ("cube_xy_center", C.c_float * 2),
                ("cube_xy_scale", C.c_float), ("cube_z_base", C.c_float), ("cube_z_range", C.c_float)]


class ReachViews(C.Structure):
    """mg_reach_views: the task-owned device tensors of FrankaReachMA."""
    _fields_ = [("cube_states", C.c_void_p), ("init_cube_states", C.c_void_p), ("dof_targets", C.c_void_p),
                ("dof_actuation", C.c_void_p)]


MG_ANYMAL_DOFS, MG_ANYMAL_OBS, MG_ANYMAL_NOISE_COLS = 12, 48, 27


class AnymalParams(C.Structure):
    """mg_anymal_params: the constants of Anymal (taskdefs.anymal_params)."""
    _fields_ = [("lin_vel_scale", C.c_float), ("ang_vel_scale", C.c_float), ("dof_pos_scale", C.c_float),
                ("dof_vel_scale", C.c_float), ("action_scale", C.c_float), ("rew_lin_vel_xy", C.c_float),
                ("rew_ang_vel_z", C.c_float), ("rew_torque", C.c_float),
                ("default_dof_pos", C.c_float * MG_ANYMAL_DOFS), ("base_init_state", C.c_float * 13),
                ("command_lo", C.c_float * 3), ("command_span", C.c_float * 3), ("base_body", C.c_int32),
                ("knee_body", C.c_int32 * 4), ("num_bodies", C.c_int32), ("clip_actions", C.c_float),
                ("clip_obs", C.c_float), ("max_episode_length", C.c_int32)]


class AnymalViews(C.Structure):
    """mg_anymal_views: the task-owned device tensors of Anymal."""
    _fields_ = [("commands", C.c_void_p), ("dof_targets", C.c_void_p)]


MG_ANYMAL_TERRAIN_OBS, MG_ANYMAL_TERRAIN_HEIGHT_POINTS, MG_ANYMAL_TERRAIN_NOISE_COLS = 188, 140, 219
MG_ANYMAL_TERRAIN_REWARDS = 13
# the columns of rew_scale, episode_sums and episode_out: the keys of the reference's episode_sums, in its order
ANYMAL_TERRAIN_REWARDS = ("lin_vel_xy", "lin_vel_z", "ang_vel_z", "ang_vel_xy", "orient", "torques", "joint_acc",
                          "base_height", "air_time", "collision", "stumble", "action_rate", "hip")


class AnymalTerrainParams(C.Structure):
    """mg_anymal_terrain_params: the constants of AnymalTerrain (taskdefs.anymal_terrain_params)."""
    _fields_ = [("lin_vel_scale", C.c_float), ("ang_vel_scale", C.c_float), ("dof_pos_scale", C.c_float),
                ("dof_vel_scale", C.c_float), ("height_meas_scale", C.c_float),
                ("rew_scale", C.c_float * MG_ANYMAL_TERRAIN_REWARDS), ("rew_termination", C.c_float),
                ("dt", C.c_float), ("Kp", C.c_float), ("Kd", C.c_float), ("action_scale", C.c_float),
                ("torque_clip", C.c_float), ("default_dof_pos", C.c_float * MG_ANYMAL_DOFS),
                ("base_init_state", C.c_float * 13), ("command_lo", C.c_float * 3), ("command_span", C.c_float * 3),
                ("base_body", C.c_int32), ("knee_body", C.c_int32 * 4), ("foot_body", C.c_int32 * 4),
                ("hip_dof", C.c_int32 * 4), ("num_bodies", C.c_int32), ("allow_knee_contacts", C.c_int32),
                ("add_noise", C.c_int32), ("noise_scale_vec", C.c_float * MG_ANYMAL_TERRAIN_OBS),
                ("max_episode_length", C.c_int32), ("max_episode_length_s", C.c_float), ("env_length", C.c_float),
                ("env_rows", C.c_int32), ("env_cols", C.c_int32), ("curriculum", C.c_int32),
                ("custom_origins", C.c_int32), ("hf_heights", C.c_void_p), ("hf_nx", C.c_int32), ("hf_ny", C.c_int32),
                ("hf_dx", C.c_float), ("hf_x0", C.c_float), ("hf_y0", C.c_float),
                ("height_points", C.c_float * (2 * MG_ANYMAL_TERRAIN_HEIGHT_POINTS)), ("clip_actions", C.c_float),
                ("clip_obs", C.c_float), ("pad_atp", C.c_int32)]


class AnymalTerrainViews(C.Structure):
    """mg_anymal_terrain_views: the task-owned device tensors of AnymalTerrain."""
    _fields_ = [("commands", C.c_void_p), ("torques", C.c_void_p), ("last_actions", C.c_void_p),
                ("last_dof_vel", C.c_void_p), ("feet_air_time", C.c_void_p), ("episode_sums", C.c_void_p),
                ("terrain_levels", C.c_void_p), ("terrain_types", C.c_void_p), ("env_origins", C.c_void_p),
                ("terrain_origins", C.c_void_p), ("dof_actuation", C.c_void_p), ("episode_out", C.c_void_p),
                ("measured_heights", C.c_void_p), ("partials", C.c_void_p), ("reset_mark", C.c_void_p),
                ("push_now", C.c_int32), ("pad_atv", C.c_int32)]


class Heightfield(C.Structure):
    """mg_heightfield: the terrain table of mg_sim_set_heightfield (device pointers, kept by the sim, not copied)."""
    _fields_ = [("heights", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("dx", C.c_float), ("x0", C.c_float),
                ("y0", C.c_float), ("hmax", C.c_float), ("env_origins", C.c_void_p)]


MG_QUAD_DOFS, MG_QUAD_BODIES, MG_QUAD_OBS, MG_QUAD_ACTIONS, MG_QUAD_NOISE_COLS = 8, 9, 21, 12, 11


class QuadcopterParams(C.Structure):
    """mg_quadcopter_params: the constants of Quadcopter (taskdefs.quadcopter_params)."""
    _fields_ = [("dof_step", C.c_float), ("thrust_step", C.c_float), ("dof_lower", C.c_float * MG_QUAD_DOFS),
                ("dof_upper", C.c_float * MG_QUAD_DOFS), ("thrust_lower", C.c_float), ("thrust_upper", C.c_float),
                ("init_root", C.c_float * 13), ("init_dof", C.c_float * (2 * MG_QUAD_DOFS)),
                ("clip_actions", C.c_float), ("clip_obs", C.c_float), ("max_episode_length", C.c_int32),
                ("rotor_body", C.c_int32 * 4)]


class QuadcopterViews(C.Structure):
    """mg_quadcopter_views: the task-owned device tensors of Quadcopter."""
    _fields_ = [("thrusts", C.c_void_p), ("dof_targets", C.c_void_p), ("forces", C.c_void_p)]


MG_AMP_DOFS, MG_AMP_BODIES, MG_AMP_OBS, MG_AMP_KEY_BODIES = 28, 15, 105, 4
MG_AMP_FRAME_FLOATS, MG_AMP_MAX_OBS_STEPS, MG_AMP_NOISE_COLS = 113, 16, 3
MG_AMP_INIT = {"Default": 0, "Start": 1, "Random": 2, "Hybrid": 3}   # HumanoidAMP.StateInit


class AmpParams(C.Structure):
    """mg_amp_params: the constants of HumanoidAMP (taskdefs.amp_params)."""
    _fields_ = [("pd_action_offset", C.c_float * MG_AMP_DOFS), ("pd_action_scale", C.c_float * MG_AMP_DOFS),
                ("motor_effort", C.c_float * MG_AMP_DOFS), ("initial_dof_pos", C.c_float * MG_AMP_DOFS),
                ("initial_root", C.c_float * 13), ("dt", C.c_double), ("power_scale", C.c_float),
                ("termination_height", C.c_float), ("hybrid_init_prob", C.c_float), ("clip_actions", C.c_float),
                ("clip_obs", C.c_float), ("max_episode_length", C.c_int32), ("enable_early_termination", C.c_int32),
                ("local_root_obs", C.c_int32), ("pd_control", C.c_int32), ("state_init", C.c_int32),
                ("num_amp_obs_steps", C.c_int32), ("key_body", C.c_int32 * MG_AMP_KEY_BODIES),
                ("contact_body_mask", C.c_uint32), ("num_bodies", C.c_int32)]


class AmpViews(C.Structure):
    """mg_amp_views: the task-owned device tensors of HumanoidAMP and its motion table (migym/motion.py)."""
    _fields_ = [("dof_targets", C.c_void_p), ("dof_actuation", C.c_void_p), ("amp_obs", C.c_void_p),
                ("terminate", C.c_void_p), ("motion_frames", C.c_void_p), ("motion_index", C.c_void_p),
                ("motion_time", C.c_void_p), ("num_motions", C.c_int32), ("num_frames", C.c_int32)]


class RenderArgs(C.Structure):
    """mg_render_args: one ray-cast of the selected envs' collision geometry (migym/render.py)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fov_y", C.c_float), ("eye_offset", C.c_float * 3),
                ("target_offset", C.c_float * 3), ("follow", C.c_int32), ("env_ids", C.c_void_p),
                ("n_sel", C.c_int32), ("num_boxes", C.c_int32), ("boxes", C.c_void_p), ("scratch", C.c_void_p),
                ("rgb", C.c_void_p), ("depth", C.c_void_p), ("ids", C.c_void_p)]


def model_bytes(spec) -> np.ndarray:
    """mg_model POD for a ModelSpec (numpy structured scalar; pass .ctypes.data)."""
    return np.ascontiguousarray(_model.pack_model(spec))


def ptr(t):
    """data_ptr of a torch tensor / numpy array, or None."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data


# ---------------------------------------------------------------------------------------------
EXPORTS = {
    "mg_last_error": (C.c_char_p, []),
    "mg_version": (C.c_int, []),
    "mg_model_sizeof": (C.c_size_t, []),
    "mg_task_params_sizeof": (C.c_size_t, []),
    "mg_task_buffers_sizeof": (C.c_size_t, []),
    "mg_sim_params_sizeof": (C.c_size_t, []),
    "mg_state_views_sizeof": (C.c_size_t, []),
    "mg_debug_phase_cycles": (C.c_int, [C.c_void_p, C.c_int32]),
    "mg_debug_phase_waves": (C.c_int, [C.c_void_p, C.c_int32]),
    "mg_debug_contacts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "mg_sim_create": (C.c_int, [C.c_void_p, C.POINTER(SimParams), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mg_sim_bind": (C.c_int, [C.c_void_p, C.POINTER(StateViews)]),
    "mg_sim_simulate": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mg_sim_set_link_forces": (C.c_int, [C.c_void_p, C.c_int32]),
    "mg_heightfield_sizeof": (C.c_size_t, []),
    "mg_sim_set_heightfield": (C.c_int, [C.c_void_p, C.POINTER(Heightfield)]),
    "mg_height_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "mg_sim_destroy": (C.c_int, [C.c_void_p]),
    "mg_set_indexed": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "mg_compute_observations": (C.c_int, [C.POINTER(TaskParams), C.c_int32] + [C.c_void_p] * 10 + [C.c_void_p]),
    "mg_compute_reward": (C.c_int, [C.POINTER(TaskParams), C.c_int32] + [C.c_void_p] * 7 + [C.c_void_p]),
    "mg_post_physics": (C.c_int, [C.c_void_p, C.POINTER(TaskParams), C.POINTER(StateViews),
                                  C.POINTER(TaskBuffers), C.c_int32, C.c_void_p]),
    "mg_pre_physics": (C.c_int, [C.c_void_p, C.POINTER(TaskParams), C.POINTER(StateViews),
                                 C.POINTER(TaskBuffers), C.c_int32, C.c_void_p]),
    "mg_env_step": (C.c_int, [C.c_void_p, C.POINTER(TaskParams), C.POINTER(TaskBuffers), C.c_void_p]),
    "mg_hand_finalize": (C.c_int, [C.POINTER(TaskParams), C.POINTER(TaskBuffers), C.c_void_p]),
    "mg_kernel_span_begin": (C.c_int, [C.c_void_p, C.c_int32]),
    "mg_kernel_span_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "mg_kernel_span_waves": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "mg_work_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32)]),
    "mg_sim_kernel_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mg_model_team_lanes": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "mg_reset_idx": (C.c_int, [C.c_void_p, C.POINTER(TaskParams), C.POINTER(TaskBuffers), C.c_void_p, C.c_int32,
                               C.c_void_p]),
    "mg_env_step_replay": (C.c_int, [C.c_void_p, C.POINTER(TaskParams), C.POINTER(TaskBuffers), C.POINTER(Replay),
                                     C.c_void_p]),
    "mg_dr_desc_sizeof": (C.c_size_t, []),
    "mg_dr_apply_args_sizeof": (C.c_size_t, []),
    "mg_dr_noise_args_sizeof": (C.c_size_t, []),
    "mg_env_props_layout": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mg_env_props_defaults": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mg_dr_apply": (C.c_int, [C.POINTER(DrApplyArgs), C.c_void_p]),
    "mg_dr_noise": (C.c_int, [C.POINTER(DrNoiseArgs), C.c_void_p]),
    "mg_sim_set_params": (C.c_int, [C.c_void_p, C.POINTER(SimParams)]),
    "mg_dynamics_bind": (C.c_int, [C.c_void_p, C.POINTER(DynamicsViews)]),
    "mg_dynamics_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mg_osc_torques": (C.c_int, [C.c_void_p, C.POINTER(OscArgs), C.c_void_p]),
    "mg_osc_args_sizeof": (C.c_size_t, []),
    "mg_reach_params_sizeof": (C.c_size_t, []),
    "mg_reach_views_sizeof": (C.c_size_t, []),
    "mg_reach_pre": (C.c_int, [C.c_void_p, C.POINTER(ReachParams), C.POINTER(ReachViews), C.POINTER(TaskBuffers),
                               C.c_void_p]),
    "mg_reach_post": (C.c_int, [C.c_void_p, C.POINTER(ReachParams), C.POINTER(ReachViews), C.POINTER(TaskBuffers),
                                C.POINTER(StateViews), C.c_void_p]),
    "mg_reach_reset_idx": (C.c_int, [C.c_void_p, C.POINTER(ReachParams), C.POINTER(ReachViews),
                                     C.POINTER(TaskBuffers), C.c_void_p, C.c_int32, C.c_void_p]),
    "mg_anymal_params_sizeof": (C.c_size_t, []),
    "mg_anymal_views_sizeof": (C.c_size_t, []),
    "mg_anymal_pre": (C.c_int, [C.c_void_p, C.POINTER(AnymalParams), C.POINTER(AnymalViews), C.POINTER(TaskBuffers),
                                C.c_void_p]),
    "mg_anymal_post": (C.c_int, [C.c_void_p, C.POINTER(AnymalParams), C.POINTER(AnymalViews), C.POINTER(TaskBuffers),
                                 C.POINTER(StateViews), C.c_void_p]),
    "mg_anymal_reset_idx": (C.c_int, [C.c_void_p, C.POINTER(AnymalParams), C.POINTER(AnymalViews),
                                      C.POINTER(TaskBuffers), C.c_void_p, C.c_int32, C.c_void_p]),
    "mg_anymal_terrain_params_sizeof": (C.c_size_t, []),
    "mg_anymal_terrain_views_sizeof": (C.c_size_t, []),
    "mg_anymal_terrain_pre": (C.c_int, [C.c_void_p, C.POINTER(AnymalTerrainParams), C.POINTER(AnymalTerrainViews),
                                        C.POINTER(TaskBuffers), C.c_void_p]),
    "mg_anymal_terrain_post": (C.c_int, [C.c_void_p, C.POINTER(AnymalTerrainParams), C.POINTER(AnymalTerrainViews),
                                         C.POINTER(TaskBuffers), C.POINTER(StateViews), C.c_void_p]),
    "mg_anymal_terrain_reset_idx": (C.c_int, [C.c_void_p, C.POINTER(AnymalTerrainParams),
                                              C.POINTER(AnymalTerrainViews), C.POINTER(TaskBuffers), C.c_void_p,
                                              C.c_int32, C.c_int32, C.c_void_p]),
    "mg_quadcopter_params_sizeof": (C.c_size_t, []),
    "mg_quadcopter_views_sizeof": (C.c_size_t, []),
    "mg_quadcopter_pre": (C.c_int, [C.c_void_p, C.POINTER(QuadcopterParams), C.POINTER(QuadcopterViews),
                                    C.POINTER(TaskBuffers), C.c_void_p]),
    "mg_quadcopter_post": (C.c_int, [C.c_void_p, C.POINTER(QuadcopterParams), C.POINTER(QuadcopterViews),
                                     C.POINTER(TaskBuffers), C.POINTER(StateViews), C.c_void_p]),
    "mg_quadcopter_reset_idx": (C.c_int, [C.c_void_p, C.POINTER(QuadcopterParams), C.POINTER(QuadcopterViews),
                                          C.POINTER(TaskBuffers), C.c_void_p, C.c_int32, C.c_void_p]),
    "mg_amp_params_sizeof": (C.c_size_t, []),
    "mg_amp_views_sizeof": (C.c_size_t, []),
    "mg_amp_pre": (C.c_int, [C.c_void_p, C.POINTER(AmpParams), C.POINTER(AmpViews), C.POINTER(TaskBuffers),
                             C.c_void_p]),
    "mg_amp_post": (C.c_int, [C.c_void_p, C.POINTER(AmpParams), C.POINTER(AmpViews), C.POINTER(TaskBuffers),
                              C.POINTER(StateViews), C.c_void_p]),
    "mg_amp_reset_idx": (C.c_int, [C.c_void_p, C.POINTER(AmpParams), C.POINTER(AmpViews), C.POINTER(TaskBuffers),
                                   C.c_void_p, C.c_int32, C.c_void_p]),
    "mg_amp_obs_demo": (C.c_int, [C.POINTER(AmpParams), C.POINTER(AmpViews), C.c_void_p, C.c_uint64, C.c_uint64,
                                  C.c_void_p, C.c_int32, C.c_void_p]),
    "mg_render_args_sizeof": (C.c_size_t, []),
    "mg_render_scratch_floats": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "mg_render": (C.c_int, [C.c_void_p, C.POINTER(RenderArgs), C.c_void_p]),
}

_LIB = None


class MigymError(RuntimeError):
    pass


def _bind(lib):
    for name, (res, args) in EXPORTS.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    return lib


def check_layout(lib):
    sizes = {"mg_model_sizeof": _model.MODEL_DTYPE.itemsize, "mg_task_params_sizeof": C.sizeof(TaskParams),
             "mg_task_buffers_sizeof": C.sizeof(TaskBuffers), "mg_sim_params_sizeof": C.sizeof(SimParams),
             "mg_state_views_sizeof": C.sizeof(StateViews), "mg_dr_desc_sizeof": C.sizeof(DrDesc),
             "mg_dr_apply_args_sizeof": C.sizeof(DrApplyArgs), "mg_dr_noise_args_sizeof": C.sizeof(DrNoiseArgs),
             "mg_osc_args_sizeof": C.sizeof(OscArgs), "mg_reach_params_sizeof": C.sizeof(ReachParams),
             "mg_reach_views_sizeof": C.sizeof(ReachViews), "mg_anymal_params_sizeof": C.sizeof(AnymalParams),
             "mg_anymal_views_sizeof": C.sizeof(AnymalViews), "mg_render_args_sizeof": C.sizeof(RenderArgs),
             "mg_amp_params_sizeof": C.sizeof(AmpParams), "mg_amp_views_sizeof": C.sizeof(AmpViews),
             "mg_quadcopter_params_sizeof": C.sizeof(QuadcopterParams),
             "mg_quadcopter_views_sizeof": C.sizeof(QuadcopterViews),
             "mg_heightfield_sizeof": C.sizeof(Heightfield),
             "mg_anymal_terrain_params_sizeof": C.sizeof(AnymalTerrainParams),
             "mg_anymal_terrain_views_sizeof": C.sizeof(AnymalTerrainViews)}
    for fn, py in sizes.items():
        c = getattr(lib, fn)()
        if c != py:
            raise MigymError(f"ABI layout mismatch: {fn}() = {c}, Python mirror = {py}")


def lib(path: str | None = None):
    """Load the HIP library (raises if it was not built)."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or os.environ.get("MIGYM_LIB", LIB_PATH)
    if not os.path.exists(p):
        raise MigymError(f"libmigym.so not found at {p}: run `python __graft_entry__.py build` "
                         "(the product path has no CPU fallback)")
    handle = _bind(C.CDLL(p))
    check_layout(handle)
    if path is None:
        _LIB = handle
    return handle


def check(rc, l=None):
    if rc != 0:
        l = l or lib()
        msg = l.mg_last_error()
        raise MigymError(f"migym call failed ({rc}): {msg.decode() if msg else ''}")
