// quadcopter_task.hpp — the task layer of Quadcopter (include/migym.h: mg_quadcopter_pre, mg_quadcopter_post,
// mg_quadcopter_reset_idx).  The step is three launches: k_quad_pre (resets, action clamp, PD targets,
// thrusts, the force tensor), the step kernels' k_simulate_xf (link forces), k_quad_post (progress, observations,
// compute_quadcopter_reward, the VecTask.step tail).
//
//   reset_idx                   quadcopter.py:280-299
//   pre_physics_step            quadcopter.py:301-330
//   post_physics_step           quadcopter.py:332-340
//   compute_observations        quadcopter.py:359-370
//   compute_quadcopter_reward   quadcopter.py:386-418
//
// Mapping: one env per lane, 64 envs per one-wave block.  A lane computes its env's rows into LDS; the block then
// stores each tensor's 64 rows, one contiguous range, over consecutive addresses (the force rows are loaded the same
// way first: the kernel writes the rotors' z components alone).  The rows a reset writes (DOF state, root row) go
// straight to memory from the env's lane: a reset is off the common path.  No atomics, no calls.  fp32 with FMA
// contraction off, in the reference's operation order, as task.hpp.
#pragma once
#include "../../include/migym.h"
#include "device_math.hpp"
#include "task.hpp"
#include "task_rows.hpp"

namespace mgq {

constexpr int kEnvs = mgt::kLanes;   // envs per block: one per lane
constexpr int kDofs = MG_QUAD_DOFS, kObs = MG_QUAD_OBS, kActs = MG_QUAD_ACTIONS, kFrc = 3 * MG_QUAD_BODIES;

#pragma clang fp contract(off)

using mgt::rand_float;
using mgt::rows_load;
using mgt::rows_store;

// draw `col` of env e's row of the (N, 11) noise layout [x | y | z | dof position 8]
__device__ __forceinline__ float quad_uniform(const mg_task_buffers& tb, int e, int col) {
  return mgt::noise_draw(tb, e, col, MG_QUAD_NOISE_COLS);
}

// reset_idx of env e (quadcopter.py:284-299): DOF state and root row written, reset and progress cleared; pos returns
// the new DOF positions
__device__ __forceinline__ void quad_reset_env(const mg_quadcopter_params& qp, const mg_task_buffers& tb, float* root_states,
                                               float* dof_state, int e, float* pos) {
  float* r = root_states + (size_t)13 * e;
  float row[13];
#pragma unroll
  for (int c = 0; c < 13; c++) row[c] = qp.init_root[c];
  row[0] = row[0] + rand_float((float)(1.5 - -1.5), -1.5f, quad_uniform(tb, e, 0));
  row[1] = row[1] + rand_float((float)(1.5 - -1.5), -1.5f, quad_uniform(tb, e, 1));
  row[2] = row[2] + rand_float((float)(1.5 - -0.2), -0.2f, quad_uniform(tb, e, 2));
#pragma unroll
  for (int c = 0; c < 13; c++) r[c] = row[c];
  float* d = dof_state + (size_t)2 * kDofs * e;
#pragma unroll
  for (int j = 0; j < kDofs; j++) {
    pos[j] = rand_float((float)(0.2 - -0.2), -0.2f, quad_uniform(tb, e, 3 + j));
    d[2 * j] = pos[j];
    d[2 * j + 1] = 0.0f;
  }
  tb.reset[e] = 0;
  tb.progress[e] = 0;
}

// pre_physics_step
__global__ __launch_bounds__(64) void k_quad_pre(mg_quadcopter_params qp, mg_quadcopter_views v, mg_task_buffers tb,
                                                 float* root_states, float* dof_state, int n_envs) {
  __shared__ float s_act[kEnvs * kActs];
  __shared__ float s_tgt[kEnvs * kDofs];
  __shared__ float s_thr[kEnvs * 4];
  __shared__ float s_frc[kEnvs * kFrc];
  const int first = blockIdx.x * kEnvs, l = threadIdx.x, e = first + l;
  const int rows = n_envs - first < kEnvs ? n_envs - first : kEnvs;
  rows_load(s_act, tb.actions + (size_t)first * kActs, rows, kActs);
  rows_load(s_tgt, v.dof_targets + (size_t)first * kDofs, rows, kDofs);
  rows_load(s_thr, v.thrusts + (size_t)first * 4, rows, 4);
  rows_load(s_frc, v.forces + (size_t)first * kFrc, rows, kFrc);
  __syncthreads();
  if (l < rows) {
    const bool was_reset = tb.reset[e] != 0;
    float pos[kDofs];
    if (was_reset) quad_reset_env(qp, tb, root_states, dof_state, e, pos);
    float* a = s_act + kActs * l;
#pragma unroll
    for (int k = 0; k < kActs; k++) a[k] = mg::clampf(a[k], qp.clip_actions);
    float* t = s_tgt + kDofs * l;
#pragma unroll
    for (int j = 0; j < kDofs; j++) {
      const float step = qp.dof_step * a[j];
      const float x = t[j] + step;
      t[j] = fmaxf(fminf(x, qp.dof_upper[j]), qp.dof_lower[j]);   // tensor_clamp: max(min(t, upper), lower)
    }
    float* th = s_thr + 4 * l;
    float* f = s_frc + kFrc * l;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float step = qp.thrust_step * a[kDofs + k];
      const float x = th[k] + step;
      th[k] = fmaxf(fminf(x, qp.thrust_upper), qp.thrust_lower);
      f[3 * qp.rotor_body[k] + 2] = th[k];
    }
    if (was_reset) {   // clear actions for reset envs (quadcopter.py:323-326)
#pragma unroll
      for (int k = 0; k < 4; k++) th[k] = 0.0f;
      for (int k = 0; k < kFrc; k++) f[k] = 0.0f;
#pragma unroll
      for (int j = 0; j < kDofs; j++) t[j] = pos[j];
    }
  }
  __syncthreads();
  if (tb.actions_out) rows_store(tb.actions_out + (size_t)first * kActs, s_act, rows, kActs);
  rows_store(v.dof_targets + (size_t)first * kDofs, s_tgt, rows, kDofs);
  rows_store(v.thrusts + (size_t)first * 4, s_thr, rows, 4);
  rows_store(v.forces + (size_t)first * kFrc, s_frc, rows, kFrc);
}

// post_physics_step + the VecTask.step tail
__global__ __launch_bounds__(64) void k_quad_post(mg_quadcopter_params qp, mg_task_buffers tb,
                                                  const float* __restrict__ root_states,
                                                  const float* __restrict__ dof_state, int n_envs) {
  __shared__ float s_root[kEnvs * 13];
  __shared__ float s_dof[kEnvs * 2 * kDofs];
  __shared__ float s_obs[kEnvs * kObs];
  __shared__ float s_rew[kEnvs];
  __shared__ float s_rst[kEnvs];
  const int first = blockIdx.x * kEnvs, l = threadIdx.x, e = first + l;
  const int rows = n_envs - first < kEnvs ? n_envs - first : kEnvs;
  rows_load(s_root, root_states + (size_t)first * 13, rows, 13);
  rows_load(s_dof, dof_state + (size_t)first * 2 * kDofs, rows, 2 * kDofs);
  __syncthreads();
  if (l < rows) {
    const long long progress = (long long)tb.progress[e] + 1;
    const float* r = s_root + 13 * l;
    float* o = s_obs + kObs * l;
    o[0] = (0.0f - r[0]) / 3.0f;
    o[1] = (0.0f - r[1]) / 3.0f;
    o[2] = (1.0f - r[2]) / 3.0f;
#pragma unroll
    for (int c = 0; c < 4; c++) o[3 + c] = r[3 + c];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      o[7 + c] = r[7 + c] / 2.0f;
      o[10 + c] = r[10 + c] / (float)M_PI;
    }
#pragma unroll
    for (int j = 0; j < kDofs; j++) o[13 + j] = s_dof[2 * kDofs * l + 2 * j];
    // compute_quadcopter_reward
    const float dz = 1.0f - r[2];
    const float dist = sqrtf(r[0] * r[0] + r[1] * r[1] + dz * dz);
    const float pos_reward = 1.0f / (1.0f + dist * dist);
    const float ez[3] = {0.0f, 0.0f, 1.0f};
    float ups[3];
    mg::t_quat_rotate(r + 3, ez, ups, false);   // quat_axis(root_quats, 2)
    const float tilt = fabsf(1.0f - ups[2]);
    const float up_reward = 1.0f / (1.0f + tilt * tilt);
    const float spin = fabsf(r[12]);
    const float spin_reward = 1.0f / (1.0f + spin * spin);
    const float rew = pos_reward + pos_reward * (up_reward + spin_reward);
    const bool die = dist > 3.0f || r[2] < 0.3f;
    const bool time_out = progress >= (long long)qp.max_episode_length - 1;
    const long long reset = (time_out || die) ? 1 : 0;
    mgt::tail_store(tb, e, rew, reset, progress, time_out);
    s_rew[l] = rew;
    s_rst[l] = (float)reset;
  }
  __syncthreads();
  mgt::block_tail(tb, s_obs, s_rew, s_rst, (size_t)first, rows, kObs, qp.clip_obs);
}

// reset_idx(env_ids): one lane per listed id.  Off the hot path (reset_done).
__global__ __launch_bounds__(64) void k_quad_reset_idx(mg_quadcopter_params qp, mg_task_buffers tb, float* root_states,
                                                       float* dof_state, const int32_t* __restrict__ ids, int n,
                                                       int n_envs) {
  const int i = blockIdx.x * kEnvs + threadIdx.x;
  if (i >= n) return;
  const int e = ids[i];
  if (e < 0 || e >= n_envs) return;
  float pos[kDofs];
  quad_reset_env(qp, tb, root_states, dof_state, e, pos);
}

#pragma clang fp contract(fast)

}  // namespace mgq
