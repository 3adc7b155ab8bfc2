// amp_task.hpp — the task layer of HumanoidAMP (include/migym.h: mg_amp_pre, mg_amp_post, mg_amp_reset_idx,
// mg_amp_obs_demo).  The step is three launches: k_amp_pre (action clamp, PD targets or efforts), the
// step kernels' k_simulate, k_amp_post (progress, observations, compute_humanoid_reset, the AMP history, the
// VecTask.step tail).
//
//   pre_physics_step / _action_to_pd_targets   amp/humanoid_amp_base.py:362-374, 419-421
//   post_physics_step                          amp/humanoid_amp_base.py:376-390, humanoid_amp.py:87-96
//   compute_humanoid_observations, dof_to_obs  amp/humanoid_amp_base.py:462-528 (= build_amp_observations,
//                                              humanoid_amp.py:299-333)
//   compute_humanoid_reset                     amp/humanoid_amp_base.py:536-562
//   reset_idx and its four StateInit modes     humanoid_amp.py:146-256
//   MotionLib.get_motion_state                 amp/utils_amp/motion_lib.py:83-153, 233-241, 265-293
//   slerp, quat_to_exp_map, exp_map_to_quat    utils/torch_jit_utils.py:422-459, 569-627
//
// Mapping: one env (reset id, demo sample) per team of 32 lanes, 2 per 64-lane block (one wave).  A team first stages
// a "state" -- root row 13, DOF positions 28, DOF velocities 28, key-body positions 12 -- in LDS, either from the
// sim's tensors or sampled from the motion table, then every lane writes its share of the 105-float observation row
// into LDS: lane j < 12 is joint j (its slerp and exp map when sampling; exp map -> quaternion -> tan-norm for a 3-DOF
// joint when observing), lanes 12..15 the four key bodies, lane 16 the root columns, lane j < 28 DOF velocity j; in
// k_amp_post lane b < 15 also tests body b's contact and height rows, combined by one wave ballot.  Rows leave LDS
// over consecutive addresses.  No atomics.  fp32 with FMA contraction off, in the reference's operation order; frame
// index, blend and motion time in fp64, rounded to fp32 once, where the reference's to_torch does it.
#pragma once
#include "../../include/migym.h"
#include "device_math.hpp"
#include "task.hpp"
#include "task_rows.hpp"

namespace mgh {

constexpr int kTeam = 32;             // lanes per env
constexpr int kEnvs = 64 / kTeam;     // envs per block
constexpr int kDofs = MG_AMP_DOFS;
constexpr int kObs = MG_AMP_OBS;
constexpr int kJoints = 12;
constexpr int kFrame = MG_AMP_FRAME_FLOATS;
constexpr int kFrameRot = 13, kFrameDofVel = 13 + 4 * MG_AMP_BODIES, kFrameKey = kFrameDofVel + kDofs;
static_assert(kFrameKey + 12 == kFrame && kObs == 13 + 52 + kDofs + 12, "frame / observation layouts");
static_assert(MG_AMP_BODIES <= kTeam && kDofs <= kTeam, "one lane per body and per DOF");

// DOF_BODY_IDS, DOF_OFFSETS (humanoid_amp_base.py:41-42) and each joint's first column in dof_to_obs's 52
__constant__ int c_joint_body[kJoints] = {1, 2, 3, 4, 6, 7, 9, 10, 11, 12, 13, 14};
__constant__ int c_joint_dof[kJoints + 1] = {0, 3, 6, 9, 10, 13, 14, 17, 18, 21, 24, 25, 28};
__constant__ int c_joint_obs[kJoints] = {0, 6, 12, 18, 19, 25, 26, 32, 33, 39, 45, 46};

// what an observation row is computed from
struct AmpSt {
  float root[13];
  float dof_pos[kDofs];
  float dof_vel[kDofs];
  float key[3 * MG_AMP_KEY_BODIES];
};

// the state tensors of the sim (bound or injected)
struct AmpState {
  float* root_states;               // (N, 13)
  float* dof_state;                 // (N*28, 2)
  const float* rigid_body_states;   // (N*15, 13)
  const float* net_contact_forces;  // (N*15, 3)
};

#pragma clang fp contract(off)

// quat_unit: x / clamp(norm(x), 1e-9)
__device__ __forceinline__ void amp_quat_unit(float* q) {
  float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  n = n > 1e-9f ? n : 1e-9f;
  q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}

// quat_from_angle_axis (torch_jit_utils.py:118-123)
__device__ __forceinline__ void amp_quat_from_angle_axis(float angle, const float* axis, float* q) {
  const float theta = angle / 2.0f;
  float n = sqrtf(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
  n = n > 1e-9f ? n : 1e-9f;
  const float s = sinf(theta);
  q[0] = (axis[0] / n) * s; q[1] = (axis[1] / n) * s; q[2] = (axis[2] / n) * s;
  q[3] = cosf(theta);
  amp_quat_unit(q);
}

// calc_heading_quat_inv (torch_jit_utils.py:655-666)
__device__ __forceinline__ void amp_heading_inv(const float* q, float* h) {
  const float ex[3] = {1.0f, 0.0f, 0.0f}, ez[3] = {0.0f, 0.0f, 1.0f};
  float d[3];
  mg::t_quat_rotate(q, ex, d, false);
  const float heading = atan2f(d[1], d[0]);
  amp_quat_from_angle_axis(-heading, ez, h);
}

// quat_to_tan_norm (torch_jit_utils.py:547-560)
__device__ __forceinline__ void amp_tan_norm(const float* q, float* o) {
  const float ex[3] = {1.0f, 0.0f, 0.0f}, ez[3] = {0.0f, 0.0f, 1.0f};
  mg::t_quat_rotate(q, ex, o, false);
  mg::t_quat_rotate(q, ez, o + 3, false);
}

// exp_map_to_quat (torch_jit_utils.py:569-592)
__device__ __forceinline__ void amp_exp_map_to_quat(const float* e, float* q) {
  float angle = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
  float axis[3] = {e[0] / angle, e[1] / angle, e[2] / angle};
  angle = mg::t_normalize_angle(angle);
  const bool mask = angle > 1e-5f;
  if (!mask) {
    angle = 0.0f;
    axis[0] = 0.0f; axis[1] = 0.0f; axis[2] = 1.0f;
  }
  amp_quat_from_angle_axis(angle, axis, q);
}

// quat_to_angle_axis (torch_jit_utils.py:422-443)
__device__ __forceinline__ void amp_quat_to_angle_axis(const float* q, float& angle, float* axis) {
  const float sin_theta = sqrtf(1.0f - q[3] * q[3]);
  angle = 2.0f * acosf(q[3]);
  angle = mg::t_normalize_angle(angle);
  const bool mask = sin_theta > 1e-5f;
  if (mask) {
    axis[0] = q[0] / sin_theta; axis[1] = q[1] / sin_theta; axis[2] = q[2] / sin_theta;
  } else {
    angle = 0.0f;
    axis[0] = 0.0f; axis[1] = 0.0f; axis[2] = 1.0f;
  }
}

// slerp (torch_jit_utils.py:594-627), with both of its special cases
__device__ __forceinline__ void amp_slerp(const float* q0, const float* q1in, float t, float* o) {
  float c = q0[3] * q1in[3] + q0[0] * q1in[0] + q0[1] * q1in[1] + q0[2] * q1in[2];
  float q1[4] = {q1in[0], q1in[1], q1in[2], q1in[3]};
  if (c < 0.0f) {
    q1[0] = -q1[0]; q1[1] = -q1[1]; q1[2] = -q1[2]; q1[3] = -q1[3];
  }
  c = fabsf(c);
  const float half_theta = acosf(c);
  const float sin_half = sqrtf(1.0f - c * c);
  const float ra = sinf((1.0f - t) * half_theta) / sin_half;
  const float rb = sinf(t * half_theta) / sin_half;
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = ra * q0[k] + rb * q1[k];
  if (fabsf(sin_half) < 0.001f) {
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = 0.5f * q0[k] + 0.5f * q1[k];
  }
  if (fabsf(c) >= 1.0f) {
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = q0[k];
  }
}

// Lane tl's share of MotionLib.get_motion_state(motion id mid, time) into s.  mid is clamped to the table.
__device__ __forceinline__ void amp_motion_state(const mg_amp_views& v, int mid, double time, int tl, AmpSt& s) {
  mid = mid < 0 ? 0 : (mid >= v.num_motions ? v.num_motions - 1 : mid);
  const int first = v.motion_index[2 * mid], nf = v.motion_index[2 * mid + 1];
  const double dt = v.motion_time[3 * mid], len = v.motion_time[3 * mid + 1];
  // _calc_frame_blend (motion_lib.py:233-241), in double as numpy has it
  double phase = time / len;
  phase = phase < 0.0 ? 0.0 : (phase > 1.0 ? 1.0 : phase);
  int i0 = (int)(phase * (double)(nf - 1));
  i0 = i0 < 0 ? 0 : (i0 > nf - 1 ? nf - 1 : i0);   // a NaN phase (a motion of zero length) must not index
  const int i1 = i0 + 1 < nf - 1 ? i0 + 1 : nf - 1;
  const float blend = (float)((time - (double)i0 * dt) / dt);
  int r0 = first + i0, r1 = first + i1;
  r0 = r0 < 0 ? 0 : (r0 >= v.num_frames ? v.num_frames - 1 : r0);
  r1 = r1 < 0 ? 0 : (r1 >= v.num_frames ? v.num_frames - 1 : r1);
  const float* f0 = v.motion_frames + (size_t)kFrame * r0;
  const float* f1 = v.motion_frames + (size_t)kFrame * r1;
  const float omb = 1.0f - blend;
  if (tl < kJoints) {   // _local_rotation_to_dof (motion_lib.py:265-293) of slerp(local_rot0, local_rot1, blend)
    const int b = c_joint_body[tl], d0 = c_joint_dof[tl], size = c_joint_dof[tl + 1] - d0;
    float q[4], angle, axis[3];
    amp_slerp(f0 + kFrameRot + 4 * b, f1 + kFrameRot + 4 * b, blend, q);
    amp_quat_to_angle_axis(q, angle, axis);
    if (size == 3) {
      s.dof_pos[d0] = angle * axis[0];
      s.dof_pos[d0 + 1] = angle * axis[1];
      s.dof_pos[d0 + 2] = angle * axis[2];
    } else {
      s.dof_pos[d0] = mg::t_normalize_angle(angle * axis[1]);
    }
  } else if (tl < kJoints + MG_AMP_KEY_BODIES) {
    const int k = tl - kJoints;
#pragma unroll
    for (int c = 0; c < 3; c++) s.key[3 * k + c] = omb * f0[kFrameKey + 3 * k + c] + blend * f1[kFrameKey + 3 * k + c];
  } else if (tl == kJoints + MG_AMP_KEY_BODIES) {
#pragma unroll
    for (int c = 0; c < 3; c++) s.root[c] = omb * f0[c] + blend * f1[c];
    amp_slerp(f0 + 3, f1 + 3, blend, s.root + 3);
#pragma unroll
    for (int c = 7; c < 13; c++) s.root[c] = f0[c];
  }
  if (tl < kDofs) s.dof_vel[tl] = f0[kFrameDofVel + tl];
}

// Lane tl's share of compute_humanoid_observations / build_amp_observations of s into row (105 floats).
__device__ __forceinline__ void amp_obs_row(const AmpSt& s, bool local_root_obs, int tl, float* row) {
  if (tl < kJoints) {   // dof_to_obs
    const int d0 = c_joint_dof[tl], size = c_joint_dof[tl + 1] - d0;
    float* o = row + 13 + c_joint_obs[tl];
    if (size == 3) {
      float q[4];
      amp_exp_map_to_quat(s.dof_pos + d0, q);
      amp_tan_norm(q, o);
    } else {
      o[0] = s.dof_pos[d0];
    }
  } else if (tl <= kJoints + MG_AMP_KEY_BODIES) {
    float h[4];
    amp_heading_inv(s.root + 3, h);
    if (tl < kJoints + MG_AMP_KEY_BODIES) {
      const int k = tl - kJoints;
      const float d[3] = {s.key[3 * k] - s.root[0], s.key[3 * k + 1] - s.root[1], s.key[3 * k + 2] - s.root[2]};
      mg::t_quat_rotate(h, d, row + 13 + 52 + kDofs + 3 * k, false);
    } else {
      row[0] = s.root[2];
      float q[4];
      if (local_root_obs) {
        mg::t_quat_mul(h, s.root + 3, q);
      } else {
        q[0] = s.root[3]; q[1] = s.root[4]; q[2] = s.root[5]; q[3] = s.root[6];
      }
      amp_tan_norm(q, row + 1);
      mg::t_quat_rotate(h, s.root + 7, row + 7, false);
      mg::t_quat_rotate(h, s.root + 10, row + 10, false);
    }
  }
  if (tl < kDofs) row[13 + 52 + tl] = s.dof_vel[tl];
}

// Lane tl's share of loading env e's state from the sim's tensors (key-body positions: rigid_body_states rows)
__device__ __forceinline__ void amp_load_state(const mg_amp_params& ap, const AmpState& st, int e, int tl, AmpSt& s,
                                               bool root_and_dofs) {
  if (root_and_dofs) {
    if (tl < kDofs) {
      const float* d = st.dof_state + (size_t)2 * ((size_t)kDofs * e + tl);
      s.dof_pos[tl] = d[0];
      s.dof_vel[tl] = d[1];
    }
    if (tl < 13) s.root[tl] = st.root_states[(size_t)13 * e + tl];
  }
  if (tl >= 16 && tl < 16 + 3 * MG_AMP_KEY_BODIES) {
    const int k = (tl - 16) / 3, c = (tl - 16) % 3;
    s.key[tl - 16] = st.rigid_body_states[(size_t)13 * ((size_t)ap.num_bodies * e + ap.key_body[k]) + c];
  }
}

// post_physics_step + the VecTask.step tail
__global__ __launch_bounds__(64) void k_amp_post(mg_amp_params ap, mg_amp_views v, mg_task_buffers tb, AmpState st,
                                                 int n_envs) {
  __shared__ AmpSt s_st[kEnvs];
  __shared__ float s_obs[kEnvs * kObs];   // the block's rows, packed
  __shared__ float s_rew[kEnvs];
  __shared__ float s_rst[kEnvs];
  const int lane = threadIdx.x, g = lane / kTeam, tl = lane % kTeam;
  const int e = blockIdx.x * kEnvs + g;
  const bool ok = e < n_envs;
  if (ok) amp_load_state(ap, st, e, tl, s_st[g], true);
  // compute_humanoid_reset's two masked any()s: lane b is body b
  bool fc = false, fh = false;
  if (ok && tl < MG_AMP_BODIES && !((ap.contact_body_mask >> tl) & 1u)) {
    const size_t row = (size_t)ap.num_bodies * e + tl;
    const float* f = st.net_contact_forces + 3 * row;
    fc = f[0] > 0.1f || f[1] > 0.1f || f[2] > 0.1f;
    fh = st.rigid_body_states[13 * row + 2] < ap.termination_height;
  }
  const unsigned long long team_bits = 0xffffffffull << (kTeam * g);
  const bool fall_contact = (__ballot(fc) & team_bits) != 0, fall_height = (__ballot(fh) & team_bits) != 0;
  __syncthreads();
  float* o = s_obs + kObs * g;
  if (ok) amp_obs_row(s_st[g], ap.local_root_obs != 0, tl, o);
  if (ok && tl == 0) {
    const long long progress = (long long)tb.progress[e] + 1;
    const bool has_fallen = fall_contact && fall_height && progress > 1;
    const long long terminated = (ap.enable_early_termination && has_fallen) ? 1 : 0;
    const bool time_out = progress >= (long long)ap.max_episode_length - 1;
    const long long reset = time_out ? 1 : terminated;
    mgt::tail_store(tb, e, 1.0f, reset, progress, time_out);
    v.terminate[e] = terminated;
    s_rew[g] = 1.0f;
    s_rst[g] = (float)reset;
  }
  __syncthreads();
  // _update_hist_amp_obs, then slot 0 = this step's row (the AMP observation is the task observation's expression)
  if (ok) {
    const int steps = ap.num_amp_obs_steps;
    float* a = v.amp_obs + (size_t)e * steps * kObs;
    for (int c = tl; c < kObs; c += kTeam) {
      for (int k = steps - 1; k >= 1; k--) a[k * kObs + c] = a[(k - 1) * kObs + c];
      a[c] = o[c];
    }
  }
  // the block's rows are one contiguous range of the output tensors
  const int first_env = blockIdx.x * kEnvs;
  const int rows = n_envs - first_env < kEnvs ? n_envs - first_env : kEnvs;
  mgt::block_tail(tb, s_obs, s_rew, s_rst, (size_t)first_env, rows, kObs, ap.clip_obs);
}

// the motion a [motion | phase] pair of uniforms selects: the first index whose cumulative weight exceeds u
// (np.random.choice), and u * length (MotionLib.sample_time)
__device__ __forceinline__ int amp_pick_motion(const mg_amp_views& v, float u) {
  int mid = 0;
  while (mid < v.num_motions - 1 && !(v.motion_time[3 * mid + 2] > (double)u)) mid++;
  return mid;
}

// reset_idx(env_ids): one team per listed id.  Off the hot path (reset_done, the constructor).
__global__ __launch_bounds__(64) void k_amp_reset_idx(mg_amp_params ap, mg_amp_views v, mg_task_buffers tb, AmpState st,
                                                      const int32_t* __restrict__ ids, int n, int n_envs) {
  __shared__ AmpSt s_st[kEnvs];
  __shared__ float s_obs[kEnvs * kObs];
  const int lane = threadIdx.x, g = lane / kTeam, tl = lane % kTeam;
  const int i = blockIdx.x * kEnvs + g;
  int e = i < n ? ids[i] : -1;
  const bool ok = e >= 0 && e < n_envs;
  if (!ok) e = 0;
  AmpSt& s = s_st[g];
  float* o = s_obs + kObs * g;
  // the draws and the path (humanoid_amp.py:151-223)
  float u[MG_AMP_NOISE_COLS];
#pragma unroll
  for (int c = 0; c < MG_AMP_NOISE_COLS; c++)
    u[c] = !ok ? 0.0f
               : (tb.noise ? tb.noise[(size_t)MG_AMP_NOISE_COLS * i + c]
                           : mg::uniform01(tb.seed, (uint64_t)(tb.env_offset + e), tb.step_counter, (uint32_t)c));
  const bool ref_path = ap.state_init == MG_AMP_INIT_START || ap.state_init == MG_AMP_INIT_RANDOM ||
                        (ap.state_init == MG_AMP_INIT_HYBRID && u[0] < ap.hybrid_init_prob);
  int mid = 0;
  double t0 = 0.0;
  if (ref_path) {   // the default path never touches the motion table (it may be absent)
    mid = amp_pick_motion(v, u[1]);
    if (ap.state_init != MG_AMP_INIT_START) t0 = (double)u[2] * v.motion_time[3 * mid + 1];
  }
  if (ok) {
    if (ref_path) {
      amp_motion_state(v, mid, t0, tl, s);
    } else {
      if (tl < kDofs) {
        s.dof_pos[tl] = ap.initial_dof_pos[tl];
        s.dof_vel[tl] = 0.0f;
      }
      if (tl < 13) s.root[tl] = ap.initial_root[tl];
    }
  }
  __syncthreads();
  if (ok) {
    // _set_env_state / _reset_default: the root row and the DOF state; the counters
    if (tl < kDofs) {
      float* d = st.dof_state + (size_t)2 * ((size_t)kDofs * e + tl);
      d[0] = s.dof_pos[tl];
      d[1] = s.dof_vel[tl];
    }
    if (tl < 13) st.root_states[(size_t)13 * e + tl] = s.root[tl];
    if (tl == kTeam - 1) {
      tb.progress[e] = 0;
      tb.reset[e] = 0;
      v.terminate[e] = 0;
    }
  }
  // the key-body positions of the env's observations are the rigid_body_states rows as bound (not refreshed); they
  // replace the motion's key positions, which nothing has read
  if (ok) amp_load_state(ap, st, e, tl, s, false);
  __syncthreads();
  if (ok) amp_obs_row(s, ap.local_root_obs != 0, tl, o);
  __syncthreads();
  const int steps = ap.num_amp_obs_steps;
  float* a = v.amp_obs + (size_t)e * steps * kObs;
  if (ok) {
    for (int c = tl; c < kObs; c += kTeam) {
      const float x = o[c];
      tb.obs[(size_t)kObs * e + c] = x;
      a[c] = x;
      if (!ref_path)   // _init_amp_obs_default
        for (int k = 1; k < steps; k++) a[k * kObs + c] = x;
    }
  }
  // _init_amp_obs_ref: slot k = build_amp_observations of the motion at t0 - dt * k (the sum in double)
  for (int k = 1; k < steps; k++) {
    __syncthreads();
    if (ok && ref_path) amp_motion_state(v, mid, t0 + -ap.dt * (double)k, tl, s);
    __syncthreads();
    if (ok && ref_path) amp_obs_row(s, ap.local_root_obs != 0, tl, o);
    __syncthreads();
    if (ok && ref_path)
      for (int c = tl; c < kObs; c += kTeam) a[k * kObs + c] = o[c];
  }
}

// fetch_amp_obs_demo: one team per sample
__global__ __launch_bounds__(64) void k_amp_obs_demo(mg_amp_params ap, mg_amp_views v, const float* __restrict__ noise,
                                                     uint64_t seed, uint64_t counter, float* __restrict__ out, int n) {
  __shared__ AmpSt s_st[kEnvs];
  __shared__ float s_obs[kEnvs * kObs];
  const int lane = threadIdx.x, g = lane / kTeam, tl = lane % kTeam;
  const int i = blockIdx.x * kEnvs + g;
  const bool ok = i < n;
  AmpSt& s = s_st[g];
  float* o = s_obs + kObs * g;
  float u[2];
#pragma unroll
  for (int c = 0; c < 2; c++)
    u[c] = !ok ? 0.0f : (noise ? noise[(size_t)2 * i + c] : mg::uniform01(seed, (uint64_t)i, counter, (uint32_t)c));
  const int mid = amp_pick_motion(v, u[0]);
  const double t0 = (double)u[1] * v.motion_time[3 * mid + 1];
  const int steps = ap.num_amp_obs_steps;
  for (int k = 0; k < steps; k++) {
    __syncthreads();
    if (ok) amp_motion_state(v, mid, t0 + -ap.dt * (double)k, tl, s);
    __syncthreads();
    if (ok) amp_obs_row(s, ap.local_root_obs != 0, tl, o);
    __syncthreads();
    if (ok)
      for (int c = tl; c < kObs; c += kTeam) out[((size_t)i * steps + k) * kObs + c] = o[c];
  }
}

// pre_physics_step: one lane per (env, DOF) element
__global__ __launch_bounds__(256) void k_amp_pre(mg_amp_params ap, const float* __restrict__ actions,
                                                 float* __restrict__ actions_out, float* __restrict__ out,
                                                 long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % kDofs);
  const float a = mg::clampf(actions[i], ap.clip_actions);
  if (actions_out) actions_out[i] = a;
  if (ap.pd_control) {
    const float scaled = ap.pd_action_scale[j] * a;
    out[i] = ap.pd_action_offset[j] + scaled;
  } else {
    const float f = a * ap.motor_effort[j];
    out[i] = f * ap.power_scale;
  }
}

#pragma clang fp contract(fast)

}  // namespace mgh
