// reach_task.hpp — the task layer of FrankaReachMA (include/migym.h: mg_reach_pre, mg_reach_post,
// mg_reach_reset_idx).  The step is three launches: k_reach_pre (action clamp and scaling + the fused
// operational-space controller of dynamics_tensors.hpp), the step kernels' k_simulate, k_reach_post (progress, the
// AND-filtered reset, observations, compute_franka_reward, the VecTask.step tail).
//
//   pre_physics_step                       franka_reach_MA.py:804-819
//   post_physics_step                      franka_reach_MA.py:821-829
//   reset_idx / _reset_init_cube_state     franka_reach_MA.py:616-679 / 681-704
//   _update_states / compute_observations  franka_reach_MA.py:519-555 / 582-612
//   compute_franka_reward                  franka_reach_MA.py:928-960
//
// k_reach_post mapping: one env per group of 8 lanes (MG_MAX_AGENTS), 8 envs per 64-lane block (one wave); lane k of a
// group is agent k when k < A and cube k when k < T.  The AND filter is a ballot masked to the group, the count of
// distinct nearest cubes an OR over the group by xor-shuffles; observation rows are staged in LDS and stored by the
// whole block over consecutive addresses (the block's 8 A rows are one contiguous range).  fp32 with FMA contraction
// off, in the reference's operation order, as task.hpp.
#pragma once
#include "../../include/migym.h"
#include "device_math.hpp"
#include "dynamics_tensors.hpp"
#include "task.hpp"
#include "task_rows.hpp"

namespace mgr {

constexpr int kGroup = MG_MAX_AGENTS;        // lanes per env
constexpr int kEnvs = 64 / kGroup;           // envs per block
constexpr int kReachDofs = 9;
constexpr int kMaxObs = 10 + 3 * MG_MAX_AGENTS + 3 * (MG_MAX_AGENTS - 1);   // 55
static_assert(kGroup == 8 && kEnvs == 8, "the lane-group reductions below are written for 8 x 8");

// the state tensors k_reach_post reads (and, on a reset, writes): the sim's bound views or the injected ones
struct ReachState {
  float* dof_state;                 // (N*A*nD, 2)
  const float* rigid_body_states;   // (N*A*nB, 13)
  const float* net_contact_forces;  // (N*A*nB, 3)
};

#pragma clang fp contract(off)

// draw `col` of env e's row of the (N, 3 T + 9) noise layout [z (T) | xy (2 T) | DOF (9)]
__device__ __forceinline__ float reach_uniform(const mg_reach_params& rp, const mg_task_buffers& tb, int e, int col) {
  return mgt::noise_draw(tb, e, col, 3 * rp.num_targets + kReachDofs);
}

// _reset_init_cube_state + the copy into _cubeA_state for cube t of env e; pos = the new position
__device__ __forceinline__ void reach_reset_cube(const mg_reach_params& rp, const mg_reach_views& v,
                                                 const mg_task_buffers& tb, int e, int t, float (&pos)[3]) {
  const int T = rp.num_targets;
  const float uz = reach_uniform(rp, tb, e, t);
  const float ux = reach_uniform(rp, tb, e, T + 2 * t), uy = reach_uniform(rp, tb, e, T + 2 * t + 1);
  pos[0] = rp.cube_xy_center[0] + rp.cube_xy_scale * (ux - 0.5f);
  pos[1] = rp.cube_xy_center[1] + rp.cube_xy_scale * (uy - 0.5f);
  pos[2] = rp.cube_z_base + uz * rp.cube_z_range;
  float* ic = v.init_cube_states + (size_t)13 * ((size_t)T * e + t);
  float* cs = v.cube_states + (size_t)13 * ((size_t)T * e + t);
#pragma unroll
  for (int c = 0; c < 13; c++) {
    const float x = c < 3 ? pos[c] : (c == 6 ? 1.0f : 0.0f);
    ic[c] = x;
    cs[c] = x;
  }
}

// the agent part of reset_idx for arm k of env e: every arm of the env gets the same 9 draws
__device__ __forceinline__ void reach_reset_arm(const mg_reach_params& rp, const mg_reach_views& v,
                                                const mg_task_buffers& tb, float* dof_state, int e, int k) {
  const int nd = rp.num_dofs, a = e * rp.num_agents + k;
  float* dof = dof_state + (size_t)2 * nd * a;
  float* tgt = v.dof_targets + (size_t)nd * a;
  float* eff = v.dof_actuation + (size_t)nd * a;
  for (int j = 0; j < nd; j++) {
    float pos = j < kReachDofs ? rp.default_dof_pos[j] : 0.0f;
    if (j < 7) {
      const float u = reach_uniform(rp, tb, e, 3 * rp.num_targets + j);
      pos = rp.default_dof_pos[j] + rp.dof_noise_scale * (u - 0.5f);
      pos = pos < rp.dof_upper[j] ? pos : rp.dof_upper[j];   // tensor_clamp: max(min(t, upper), lower)
      pos = pos > rp.dof_lower[j] ? pos : rp.dof_lower[j];
    }
    dof[2 * j] = pos;
    dof[2 * j + 1] = 0.0f;
    tgt[j] = pos;
    eff[j] = 0.0f;
  }
  tb.progress[a] = 0;
  tb.reset[a] = 0;
}

// post_physics_step + the VecTask.step tail; n_envs envs of rp.num_agents arms
__global__ __launch_bounds__(64) void k_reach_post(mg_reach_params rp, mg_reach_views v, mg_task_buffers tb,
                                                   ReachState st, int n_envs) {
  __shared__ float s_cube[kEnvs][3 * MG_MAX_AGENTS];
  __shared__ float s_eef[kEnvs][MG_MAX_AGENTS][3];
  __shared__ float s_obs[kEnvs * MG_MAX_AGENTS * kMaxObs];   // the block's rows, packed: row r at r * num_obs
  __shared__ float s_rew[64];
  __shared__ float s_rst[64];
  const int lane = threadIdx.x, g = lane / kGroup, k = lane % kGroup;
  const int A = rp.num_agents, T = rp.num_targets, no = rp.num_obs, nb = rp.num_bodies;
  const int e = blockIdx.x * kEnvs + g;
  const bool env_ok = e < n_envs;
  const bool agent = env_ok && k < A;
  const int a = agent ? e * A + k : 0;
  // 1. progress += 1
  long long progress = agent ? (long long)tb.progress[a] + 1 : 0;
  long long reset = agent ? (long long)tb.reset[a] : 0;
  // 2. the AND filter over the env's agents: a ballot masked to the lane group
  const unsigned long long done = __ballot(agent && reset != 0);
  const unsigned full = (1u << A) - 1u;
  const bool do_reset = env_ok && ((unsigned)(done >> (g * kGroup)) & full) == full;
  float cpos[3] = {0.0f, 0.0f, 0.0f};
  if (env_ok && k < T) {
    if (do_reset) {
      reach_reset_cube(rp, v, tb, e, k, cpos);
    } else {
      const float* cs = v.cube_states + (size_t)13 * ((size_t)T * e + k);
      cpos[0] = cs[0]; cpos[1] = cs[1]; cpos[2] = cs[2];
    }
    s_cube[g][3 * k + 0] = cpos[0]; s_cube[g][3 * k + 1] = cpos[1]; s_cube[g][3 * k + 2] = cpos[2];
  }
  if (agent && do_reset) {
    reach_reset_arm(rp, v, tb, st.dof_state, e, k);
    progress = 0;
    reset = 0;
  }
  // 3. the end effector as simulate left it (not recomputed after a reset)
  float ep[3] = {0.0f, 0.0f, 0.0f}, eq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (agent) {
    const float* row = st.rigid_body_states + (size_t)13 * ((size_t)nb * a + rp.eef_body);
    ep[0] = row[0]; ep[1] = row[1]; ep[2] = row[2];
    eq[0] = row[3]; eq[1] = row[4]; eq[2] = row[5]; eq[3] = row[6];
    s_eef[g][k][0] = ep[0]; s_eef[g][k][1] = ep[1]; s_eef[g][k][2] = ep[2];
  }
  __syncthreads();
  // nearest cube: argmin of |c - a|, the first index on ties
  int near = 0;
  float rel[3] = {0.0f, 0.0f, 0.0f};
  if (agent) {
    float best = 0.0f;
    for (int c = 0; c < T; c++) {
      const float dx = s_cube[g][3 * c] - ep[0], dy = s_cube[g][3 * c + 1] - ep[1], dz = s_cube[g][3 * c + 2] - ep[2];
      const float d = sqrtf(dx * dx + dy * dy + dz * dz);
      if (c == 0 || d < best) {
        best = d; near = c;
        rel[0] = dx; rel[1] = dy; rel[2] = dz;
      }
    }
  }
  // the number of distinct nearest-cube ids among the env's agents: OR of one-hot masks over the 8-lane group
  unsigned hot = agent ? (1u << near) : 0u;
  hot |= __shfl_xor(hot, 1);
  hot |= __shfl_xor(hot, 2);
  hot |= __shfl_xor(hot, 4);
  const int touched = __popc(hot);
  // 4. the observation row into the block's packed LDS rows
  float rew = 0.0f;
  if (agent) {
    float* o = s_obs + (size_t)no * (g * A + k);
    int c = 0;
    for (int i = 0; i < 3 * T; i++) o[c++] = s_cube[g][i];
    for (int i = 0; i < 4; i++) o[c++] = eq[i];
    for (int i = 0; i < 3; i++) o[c++] = ep[i];
    for (int i = 0; i < 3; i++) o[c++] = rel[i];
    for (int j = 1; j < A; j++) {
      const int src = (k + j) % A;
      for (int i = 0; i < 3; i++) o[c++] = s_eef[g][src][i];
    }
    // 5. compute_franka_reward
    const float d = sqrtf(rel[0] * rel[0] + rel[1] * rel[1] + rel[2] * rel[2]);
    const float dist_reward = 1.0f / (0.5f + d * d);
    float ac = 0.0f;
    for (int i = 0; i < 6; i++) {
      const float x = mg::clampf(tb.actions[(size_t)6 * a + i], rp.clip_actions);
      ac += x * x;
    }
    rew = dist_reward - ac * 0.01f;
    const float all_touched = (float)touched / (float)A;
    const float* hf = st.net_contact_forces + (size_t)3 * ((size_t)nb * a + rp.hand_body);
    const float fn = sqrtf(hf[0] * hf[0] + hf[1] * hf[1] + hf[2] * hf[2]);
    const float punish = fn >= 0.1f ? -10.0f : 0.0f;
    rew = rew + (all_touched + punish);
    rew = rew > 0.0f ? rew : 0.0f;
    const float max_ep_m1 = (float)rp.max_episode_length - 1.0f;
    if ((float)progress >= max_ep_m1) reset = 1;
    // 6. the VecTask.step tail
    mgt::tail_store(tb, a, rew, reset, progress, (float)progress >= max_ep_m1);
    s_rew[g * A + k] = rew;   // by packed row, as s_obs
    s_rst[g * A + k] = (float)reset;
  }
  __syncthreads();
  // the block's rows are one contiguous range of the output tensors
  const int first_env = blockIdx.x * kEnvs;
  const int envs_here = n_envs - first_env < kEnvs ? n_envs - first_env : kEnvs;
  mgt::block_tail(tb, s_obs, s_rew, s_rst, (size_t)first_env * A, envs_here * A, no, rp.clip_obs);
}

// reset_idx(agent_ids): each block counts, in LDS, the ids that fall into its 256 envs (bincount(ids // A)), then one
// lane per env applies the reset where the count reaches A.  Off the hot path (the constructor, evaluation resets).
__global__ __launch_bounds__(256) void k_reach_reset_idx(mg_reach_params rp, mg_reach_views v, mg_task_buffers tb,
                                                         float* dof_state, const int32_t* __restrict__ ids, int n,
                                                         int n_envs) {
  __shared__ int cnt[256];
  const int base = blockIdx.x * 256, A = rp.num_agents;
  cnt[threadIdx.x] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) {
    const int id = ids[i];
    if (id < 0 || id >= n_envs * A) continue;
    const int le = id / A - base;
    if (le >= 0 && le < 256) atomicAdd(&cnt[le], 1);
  }
  __syncthreads();
  const int e = base + threadIdx.x;
  if (e >= n_envs || cnt[threadIdx.x] < A) return;
  float pos[3];
  for (int t = 0; t < rp.num_targets; t++) reach_reset_cube(rp, v, tb, e, t, pos);
  for (int k = 0; k < A; k++) reach_reset_arm(rp, v, tb, dof_state, e, k);
}

#pragma clang fp contract(fast)

// pre_physics_step: the team kernel of mg_osc_torques with dpose taken from the action rows
__global__ __launch_bounds__(64) void k_reach_pre(const mgd::DynModel* __restrict__ gm, int n, mgd::OscParams p,
                                                  mgd::OscActions oa, const float* __restrict__ root_states,
                                                  const float* __restrict__ dof_state,
                                                  const float* __restrict__ env_props, int props_stride) {
  mgd::osc_team<true>(gm, n, p, root_states, dof_state, env_props, props_stride, &oa);
}

}  // namespace mgr
