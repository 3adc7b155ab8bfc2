// anymal_task.hpp — the task layer of Anymal (include/migym.h: mg_anymal_pre, mg_anymal_post, mg_anymal_reset_idx;
// DESIGN.md §11).  The step is three launches: k_anymal_pre (action clamp, PD targets), the step kernels' k_simulate,
// k_anymal_post (progress, resets, observations, compute_anymal_reward, the VecTask.step tail).
//
//   pre_physics_step              anymal.py:226-229
//   post_physics_step             anymal.py:231-239
//   reset_idx                     anymal.py:278-304
//   compute_anymal_reward         anymal.py:311-351
//   compute_anymal_observations   anymal.py:354-386
//
// k_anymal_post mapping: one env per team of 16 lanes, 4 envs per 64-lane block (one wave); lane j < 12 of a team is
// DOF column j (its dof_pos / dof_vel / action / torque), lanes 12..14 hold command x / y / yaw, lanes 12..15 the four
// THIGH contact rows, lane 15 the root row of a reset.  Σ torque² and the knee maximum are xor-shuffle butterflies
// inside the team (registers only, every lane ends with the result); observation rows are staged in LDS and stored by
// the whole block over consecutive addresses (the block's 4 rows are one contiguous range).  No atomics.  fp32 with
// FMA contraction off, in the reference's operation order, as task.hpp.
#pragma once
#include "../../include/migym.h"
#include "device_math.hpp"
#include "task.hpp"
#include "task_rows.hpp"

namespace mga {

constexpr int kTeam = 16;              // lanes per env
constexpr int kEnvs = 64 / kTeam;      // envs per block
constexpr int kDofs = MG_ANYMAL_DOFS;
constexpr int kObs = MG_ANYMAL_OBS;
static_assert(kDofs + 4 == kTeam && kObs == 12 + 3 * kDofs, "the lane roles below are written for 12 DOFs in 16 lanes");

// the state tensors k_anymal_post reads (and, on a reset, writes): the sim's bound views or the injected ones
struct AnymalState {
  float* root_states;               // (N, 13)
  float* dof_state;                 // (N*12, 2)
  const float* dof_force;           // (N, 12)
  const float* net_contact_forces;  // (N*nB, 3)
};

#pragma clang fp contract(off)

// draw `col` of env e's row of the (N, 27) noise layout [positions_offset 12 | velocities 12 | cmd x | y | yaw]
__device__ __forceinline__ float anymal_uniform(const mg_task_buffers& tb, int e, int col) {
  return mgt::noise_draw(tb, e, col, MG_ANYMAL_NOISE_COLS);
}

// lane `tl` of env e's team applies its share of reset_idx (anymal.py:283-303): DOF tl's position and velocity, command
// tl - 12, the root row (lane 15).  pos / vel / cmd return what the lane wrote.
__device__ __forceinline__ void anymal_reset_lane(const mg_anymal_params& ap, const mg_anymal_views& v,
                                                  const mg_task_buffers& tb, const AnymalState& st, int e, int tl,
                                                  float& pos, float& vel, float& cmd) {
  if (tl < kDofs) {
    pos = ap.default_dof_pos[tl] * mgt::rand_float((float)(1.5 - 0.5), 0.5f, anymal_uniform(tb, e, tl));
    vel = mgt::rand_float((float)(0.1 - -0.1), -0.1f, anymal_uniform(tb, e, kDofs + tl));
    float* d = st.dof_state + (size_t)2 * ((size_t)kDofs * e + tl);
    d[0] = pos;
    d[1] = vel;
  } else if (tl < kDofs + 3) {
    const int c = tl - kDofs;
    cmd = mgt::rand_float(ap.command_span[c], ap.command_lo[c], anymal_uniform(tb, e, 2 * kDofs + c));
    v.commands[(size_t)3 * e + c] = cmd;
  } else {
    float* r = st.root_states + (size_t)13 * e;
#pragma unroll
    for (int c = 0; c < 13; c++) r[c] = ap.base_init_state[c];
  }
}

// xor-shuffle butterflies inside the 16-lane team: every lane ends with the team's result.  The DPP forms of these
// (mg::team_sum in team_physics.hpp, mg::team_max_dpp in hull.hpp) belong to the step kernels' translation units:
// migym.hip includes neither header, team_physics.hpp is to stay as it is, and pulling its templates and fp-contract
// pragmas into this translation unit for two 4-step reductions per env would put the other kernels' code objects at
// stake.  reach_task.hpp reduces the same way.  The kernel is bound by its bytes.
__device__ __forceinline__ float team16_sum(float x) {
  x += __shfl_xor(x, 1);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 8);
  return x;
}
__device__ __forceinline__ float team16_max(float x) {
  x = fmaxf(x, __shfl_xor(x, 1));
  x = fmaxf(x, __shfl_xor(x, 2));
  x = fmaxf(x, __shfl_xor(x, 4));
  x = fmaxf(x, __shfl_xor(x, 8));
  return x;
}

// post_physics_step + the VecTask.step tail
__global__ __launch_bounds__(64) void k_anymal_post(mg_anymal_params ap, mg_anymal_views v, mg_task_buffers tb,
                                                    AnymalState st, int n_envs) {
  __shared__ float s_obs[kEnvs * kObs];   // the block's rows, packed
  __shared__ float s_cmd[kEnvs][4];
  __shared__ float s_rew[kEnvs];
  __shared__ float s_rst[kEnvs];
  const int lane = threadIdx.x, g = lane / kTeam, tl = lane % kTeam;
  const int e = blockIdx.x * kEnvs + g;
  const bool ok = e < n_envs;
  const int ee = ok ? e : 0;
  // 1. progress += 1; the envs whose reset flag is set are reset now
  long long progress = (long long)tb.progress[ee] + 1;
  const bool do_reset = ok && tb.reset[ee] != 0;
  float pos = 0.0f, vel = 0.0f, cmd = 0.0f;
  if (do_reset) {
    anymal_reset_lane(ap, v, tb, st, e, tl, pos, vel, cmd);
    progress = 0;
  } else if (ok) {
    if (tl < kDofs) {
      const float* d = st.dof_state + (size_t)2 * ((size_t)kDofs * e + tl);
      pos = d[0];
      vel = d[1];
    } else if (tl < kDofs + 3) {
      cmd = v.commands[(size_t)3 * e + (tl - kDofs)];
    }
  }
  if (tl >= kDofs && tl < kDofs + 3) s_cmd[g][tl - kDofs] = cmd;
  // 2. per-DOF columns and the two team reductions
  float tq2 = 0.0f, knee = 0.0f;
  float* o = s_obs + kObs * g;
  if (ok && tl < kDofs) {
    const float a = mg::clampf(tb.actions[(size_t)kDofs * e + tl], ap.clip_actions);
    o[12 + tl] = (pos - ap.default_dof_pos[tl]) * ap.dof_pos_scale;
    o[24 + tl] = vel * ap.dof_vel_scale;
    o[36 + tl] = a;
    const float t = st.dof_force[(size_t)kDofs * e + tl];
    tq2 = t * t;
  } else if (ok) {
    const float* f = st.net_contact_forces + (size_t)3 * ((size_t)ap.num_bodies * e + ap.knee_body[tl - kDofs]);
    knee = sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  }
  tq2 = team16_sum(tq2);
  knee = team16_max(knee);
  __syncthreads();
  // 3. the root-frame columns, compute_anymal_reward and the tail: lane 0 of the team
  if (ok && tl == 0) {
    float root[13];
    if (do_reset) {
#pragma unroll
      for (int c = 0; c < 13; c++) root[c] = ap.base_init_state[c];
    } else {
      const float* r = st.root_states + (size_t)13 * e;
#pragma unroll
      for (int c = 0; c < 13; c++) root[c] = r[c];
    }
    const float grav[3] = {0.0f, 0.0f, -1.0f};
    float lin[3], ang[3], pg[3];
    mg::t_quat_rotate(root + 3, root + 7, lin, true);
    mg::t_quat_rotate(root + 3, root + 10, ang, true);
    mg::t_quat_rotate(root + 3, grav, pg, false);
    const float c0 = s_cmd[g][0], c1 = s_cmd[g][1], c2 = s_cmd[g][2];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      o[i] = lin[i] * ap.lin_vel_scale;
      o[3 + i] = ang[i] * ap.ang_vel_scale;
      o[6 + i] = pg[i];
    }
    o[9] = c0 * ap.lin_vel_scale;
    o[10] = c1 * ap.lin_vel_scale;
    o[11] = c2 * ap.ang_vel_scale;
    const float d0 = c0 - lin[0], d1 = c1 - lin[1], d2 = c2 - ang[2];
    const float lin_err = d0 * d0 + d1 * d1, ang_err = d2 * d2;
    const float rew_lin = expf(-lin_err / 0.25f) * ap.rew_lin_vel_xy;
    const float rew_ang = expf(-ang_err / 0.25f) * ap.rew_ang_vel_z;
    const float rew_tq = tq2 * ap.rew_torque;
    float rew = rew_lin + rew_ang + rew_tq;
    rew = rew > 0.0f ? rew : 0.0f;
    const float* bf = st.net_contact_forces + (size_t)3 * ((size_t)ap.num_bodies * e + ap.base_body);
    const float base = sqrtf(bf[0] * bf[0] + bf[1] * bf[1] + bf[2] * bf[2]);
    const bool time_out = progress >= (long long)ap.max_episode_length - 1;
    const long long reset = (base > 1.0f || knee > 1.0f || time_out) ? 1 : 0;
    mgt::tail_store(tb, e, rew, reset, progress, time_out);
    s_rew[g] = rew;
    s_rst[g] = (float)reset;
  }
  __syncthreads();
  // 4. the block's rows are one contiguous range of the output tensors
  const int first_env = blockIdx.x * kEnvs;
  const int rows = n_envs - first_env < kEnvs ? n_envs - first_env : kEnvs;
  mgt::block_tail(tb, s_obs, s_rew, s_rst, (size_t)first_env, rows, kObs, ap.clip_obs);
}

// reset_idx(env_ids): one 16-lane team per listed id.  Off the hot path (the constructor, reset_done).
__global__ __launch_bounds__(64) void k_anymal_reset_idx(mg_anymal_params ap, mg_anymal_views v, mg_task_buffers tb,
                                                         AnymalState st, const int32_t* __restrict__ ids, int n,
                                                         int n_envs) {
  const int i = blockIdx.x * kEnvs + threadIdx.x / kTeam, tl = threadIdx.x % kTeam;
  if (i >= n) return;
  const int e = ids[i];
  if (e < 0 || e >= n_envs) return;
  float pos, vel, cmd;
  anymal_reset_lane(ap, v, tb, st, e, tl, pos, vel, cmd);
  if (tl == kTeam - 1) {
    tb.progress[e] = 0;
    tb.reset[e] = 1;   // anymal.py:304
  }
}

// pre_physics_step: one lane per (env, DOF) element
__global__ __launch_bounds__(256) void k_anymal_pre(mg_anymal_params ap, const float* __restrict__ actions,
                                                    float* __restrict__ actions_out, float* __restrict__ targets,
                                                    long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float a = mg::clampf(actions[i], ap.clip_actions);
  if (actions_out) actions_out[i] = a;
  const float scaled = ap.action_scale * a;
  targets[i] = scaled + ap.default_dof_pos[(int)(i % kDofs)];
}

#pragma clang fp contract(fast)

}  // namespace mga
