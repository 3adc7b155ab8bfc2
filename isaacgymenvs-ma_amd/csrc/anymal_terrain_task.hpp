// anymal_terrain_task.hpp — the task layer of AnymalTerrain (include/migym.h: mg_anymal_terrain_pre, _post,
// _reset_idx).  A control step is (k_at_pre, k_simulate_hf) x decimation, k_at_post, k_at_finish.
//
//   pre_physics_step      anymal_terrain.py:441-451
//   post_physics_step     anymal_terrain.py:453-485
//   check_termination     anymal_terrain.py:294-300
//   compute_reward        anymal_terrain.py:315-382
//   reset_idx             anymal_terrain.py:384-425
//   update_terrain_level  anymal_terrain.py:427-435
//   compute_observations  anymal_terrain.py:302-313, get_heights 515-538
//
// k_at_post mapping: one env per team of 16 lanes, 4 envs per 64-lane block (one wave), as k_anymal_post.  Lane j < 12
// of a team is DOF column j (position, velocity, action, torque, last action, last velocity); lanes 12..15 are the four
// knee / foot contact rows and feet_air_time columns; lane 0 also carries the root row (base-frame velocities, heading,
// termination, the 13 reward terms), lane 15 the curriculum and the root row of a reset, lanes 12..14 the new commands.
// The 140 height gathers of an env go round its 16 lanes (9 each), and so do the 13 episode sums and the 188 noise
// columns.  Sums over DOFs and feet are xor-shuffle butterflies inside the team; the phases meet in LDS, and the block's
// four observation rows leave LDS as one contiguous range (mgt::block_tail).  The means over envs are two-stage and in a
// fixed order: every block leaves its partial sums in views.partials, k_at_finish adds them up.  No atomics.  fp32 with
// FMA contraction off, in the reference's operation order, as task.hpp; the height scan's cell is the one expression
// that keeps the default contraction, as k_height_scan (height_scan.hip) has it.
#pragma once
#include "../../include/migym.h"
#include "device_math.hpp"
#include "task.hpp"
#include "task_rows.hpp"

namespace mgat {

constexpr int kTeam = 16;
constexpr int kEnvs = 64 / kTeam;
constexpr int kDofs = MG_ANYMAL_DOFS;
constexpr int kObs = MG_ANYMAL_TERRAIN_OBS;
constexpr int kPts = MG_ANYMAL_TERRAIN_HEIGHT_POINTS;
constexpr int kRew = MG_ANYMAL_TERRAIN_REWARDS;
constexpr int kCols = MG_ANYMAL_TERRAIN_NOISE_COLS;
constexpr int kPart = 16;   // floats of a block's partial row: 13 sums | resets | terrain levels | unused
// the noise row's columns
constexpr int kColPush = 0, kColPos = 2, kColVel = 14, kColRoot = 26, kColCmd = 28, kColObs = 31;
static_assert(kColObs + kObs == kCols && kObs == 36 + kPts + kDofs, "the 219-column draw order");

struct State {
  float* root_states;               // (N, 13), world coordinates
  float* dof_state;                 // (N*12, 2)
  const float* net_contact_forces;  // (N*nB, 3)
};

// get_heights' cell (k_height_scan's expression, default FMA contraction as there): the table height under the point
// (px, py) of the yaw frame of the root row r; both cell indices clamped, so every read is inside the table
__device__ __forceinline__ float scan_height(const mg_anymal_terrain_params& ap, const float* r, float px, float py) {
  const float qz = r[5], qw = r[6];
  const float il = 1.0f / sqrtf(qz * qz + qw * qw);
  const float z = qz * il, w = qw * il;
  const float c = w * w - z * z, s = 2.0f * w * z;
  const float X = (c * px - s * py) + r[0], Y = (s * px + c * py) + r[1];
  int ix = (int)((X - ap.hf_x0) / ap.hf_dx), iy = (int)((Y - ap.hf_y0) / ap.hf_dx);
  ix = ix < 0 ? 0 : (ix > ap.hf_nx - 2 ? ap.hf_nx - 2 : ix);
  iy = iy < 0 ? 0 : (iy > ap.hf_ny - 2 ? ap.hf_ny - 2 : iy);
  const float* h = ap.hf_heights + (size_t)ix * ap.hf_ny + iy;
  return fminf(h[0], h[ap.hf_ny + 1]);
}

#pragma clang fp contract(off)

__device__ __forceinline__ float draw(const mg_task_buffers& tb, int e, int col) {
  return mgt::noise_draw(tb, e, col, kCols);
}

__device__ __forceinline__ float team16_sum(float x) {
  x += __shfl_xor(x, 1);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 8);
  return x;
}

__device__ __forceinline__ float norm3(const float* f) { return sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]); }

// quat_apply (torch_jit_utils): b + w * t + xyz x t, t = 2 (xyz x b)
__device__ __forceinline__ void quat_apply(const float* q, const float* b, float* o) {
  const float t0 = (q[1] * b[2] - q[2] * b[1]) * 2.0f, t1 = (q[2] * b[0] - q[0] * b[2]) * 2.0f,
              t2 = (q[0] * b[1] - q[1] * b[0]) * 2.0f;
  o[0] = b[0] + q[3] * t0 + (q[1] * t2 - q[2] * t1);
  o[1] = b[1] + q[3] * t1 + (q[2] * t0 - q[0] * t2);
  o[2] = b[2] + q[3] * t2 + (q[0] * t1 - q[1] * t0);
}

// wrap_to_pi (anymal_terrain.py:684-687) as the scripted function runs: TorchScript compiles its `angles %= 2 pi` to
// fmod_, the truncated remainder, not Python's floored one, so an angle below -pi is not wrapped (a reference quirk,
// kept: DESIGN.md §16); then -2 pi above pi
__device__ __forceinline__ float wrap_to_pi(float a) {
  const float two_pi = 6.283185307179586f;
  float m = fmodf(a, two_pi);
  if (m > 3.141592653589793f) m -= two_pi;
  return m;
}

// What the teams of a block share through LDS.
struct Shared {
  float obs[kEnvs * kObs];
  float term[kEnvs][kPart];     // the 13 reward terms of this step
  float sums[kEnvs][kPart];     // the episode sums a reset env gives up | its reset flag | its terrain level
  float root[kEnvs][13];        // the root row the observations see (post-reset)
  float cmd[kEnvs][4];
  float rew[kEnvs], rst[kEnvs];
  int reset[kEnvs];
};

// The reset of env e by its team (anymal_terrain.py:384-425 without the extras): lanes < 12 the DOF draws, lanes 12..14
// the commands, lane 15 the curriculum and the root row.  root / cmd: the team's LDS rows, holding the pre-reset root
// row and the old commands on entry and the new ones on return.  Every lane of the block must call it (it holds block
// barriers), after a barrier that follows the rows' writes; it ends with one.  pos / vel: the lane's DOF state.
__device__ __forceinline__ void reset_team(const mg_anymal_terrain_params& ap, const mg_anymal_terrain_views& v,
                                           const mg_task_buffers& tb, const State& st, int e, int tl, bool on,
                                           bool update_levels, float* root, float* cmd, float& pos, float& vel) {
  if (on && tl < kDofs) {
    pos = ap.default_dof_pos[tl] * mgt::rand_float((float)(1.5 - 0.5), 0.5f, draw(tb, e, kColPos + tl));
    vel = mgt::rand_float((float)(0.1 - -0.1), -0.1f, draw(tb, e, kColVel + tl));
    float* d = st.dof_state + (size_t)2 * ((size_t)kDofs * e + tl);
    d[0] = pos;
    d[1] = vel;
  }
  float c_new = 0.0f;
  if (on && tl >= kDofs && tl < kDofs + 3) {
    const int c = tl - kDofs;
    c_new = mgt::rand_float(ap.command_span[c], ap.command_lo[c], draw(tb, e, kColCmd + c));
  }
  if (on && tl == kTeam - 1) {
    float* o = v.env_origins + (size_t)3 * e;
    if (ap.custom_origins) {
      if (update_levels && ap.curriculum) {
        // update_terrain_level, with the norm of this env's own commands (the reference's torch.norm has no dim and so
        // takes every env that resets with it: INTEGRATION.md)
        const float dx = root[0] - o[0], dy = root[1] - o[1];
        const float dist = sqrtf(dx * dx + dy * dy);
        const float cn = sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1]);
        int level = v.terrain_levels[e];
        level -= dist < cn * ap.max_episode_length_s * 0.25f ? 1 : 0;
        level += dist > ap.env_length * 0.5f ? 1 : 0;
        level = (level < 0 ? 0 : level) % ap.env_rows;
        v.terrain_levels[e] = level;
        int type = v.terrain_types[e];
        type = type < 0 ? 0 : (type >= ap.env_cols ? ap.env_cols - 1 : type);
        const float* t = v.terrain_origins + (size_t)3 * ((size_t)level * ap.env_cols + type);
        o[0] = t[0];
        o[1] = t[1];
        o[2] = t[2];
      }
#pragma unroll
      for (int c = 0; c < 13; c++) root[c] = ap.base_init_state[c];
      root[0] += o[0];
      root[1] += o[1];
      root[2] += o[2];
      root[0] += mgt::rand_float((float)(0.5 - -0.5), -0.5f, draw(tb, e, kColRoot));
      root[1] += mgt::rand_float((float)(0.5 - -0.5), -0.5f, draw(tb, e, kColRoot + 1));
    } else {
#pragma unroll
      for (int c = 0; c < 13; c++) root[c] = ap.base_init_state[c];
    }
    float* r = st.root_states + (size_t)13 * e;
#pragma unroll
    for (int c = 0; c < 13; c++) r[c] = root[c];
  }
  __syncthreads();   // the old commands have been read
  if (on && tl >= kDofs && tl < kDofs + 3) cmd[tl == kDofs + 2 ? 3 : tl - kDofs] = c_new;
  __syncthreads();
  if (on && tl >= kDofs && tl < kTeam) {
    // commands[env_ids] *= norm(commands[env_ids, :2]) > 0.25: the whole row, the yaw rate included
    const int c = tl - kDofs;
    const bool keep = sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1]) > 0.25f;
    const float x = cmd[c] * (keep ? 1.0f : 0.0f);
    v.commands[(size_t)4 * e + c] = x;
    v.feet_air_time[(size_t)4 * e + c] = 0.0f;
    cmd[c] = x;   // after the four lanes' reads above: one wave, LDS in program order
  }
  __syncthreads();
}

// a block's row of views.partials from the LDS rows of its envs, by lanes < kPart in env order
__device__ __forceinline__ void store_partials(const mg_anymal_terrain_views& v, const Shared& s, int rows) {
  const int c = threadIdx.x;
  if (c >= kPart) return;
  float acc = 0.0f;
  for (int g = 0; g < rows; g++) acc += (c < kRew && s.reset[g] == 0) ? 0.0f : s.sums[g][c];
  v.partials[(size_t)kPart * blockIdx.x + c] = acc;
}

// post_physics_step + the VecTask.step tail
__global__ __launch_bounds__(64) void k_at_post(mg_anymal_terrain_params ap, mg_anymal_terrain_views v,
                                                mg_task_buffers tb, State st, int n_envs) {
  __shared__ Shared s;
  const int lane = threadIdx.x, g = lane / kTeam, tl = lane % kTeam;
  const int e = blockIdx.x * kEnvs + g;
  const bool ok = e < n_envs;
  const int ee = ok ? e : 0;
  // ---- the lane's own columns
  float pos = 0.0f, vel = 0.0f, act = 0.0f;
  float tq2 = 0.0f, acc2 = 0.0f, rate2 = 0.0f, hip = 0.0f, knee = 0.0f, stumble = 0.0f, air = 0.0f;
  if (ok && tl < kDofs) {
    const size_t i = (size_t)kDofs * e + tl;
    pos = st.dof_state[2 * i];
    vel = st.dof_state[2 * i + 1];
    act = mg::clampf(tb.actions[i], ap.clip_actions);
    const float t = v.torques[i];
    tq2 = t * t;
    const float da = v.last_dof_vel[i] - vel;
    acc2 = da * da;
    const float dr = v.last_actions[i] - act;
    rate2 = dr * dr;
    if (tl == ap.hip_dof[0] || tl == ap.hip_dof[1] || tl == ap.hip_dof[2] || tl == ap.hip_dof[3])
      hip = fabsf(pos - ap.default_dof_pos[tl]);
  } else if (ok) {
    const int k = tl - kDofs;
    const float* kf = st.net_contact_forces + (size_t)3 * ((size_t)ap.num_bodies * e + ap.knee_body[k]);
    knee = norm3(kf) > 1.0f ? 1.0f : 0.0f;
    const float* ff = st.net_contact_forces + (size_t)3 * ((size_t)ap.num_bodies * e + ap.foot_body[k]);
    stumble = (sqrtf(ff[0] * ff[0] + ff[1] * ff[1]) > 5.0f && fabsf(ff[2]) < 1.0f) ? 1.0f : 0.0f;
    // the air-time reward and the feet_air_time update (anymal_terrain.py:351-356)
    const bool contact = ff[2] > 1.0f;
    float t = v.feet_air_time[(size_t)4 * e + k];
    const bool first = t > 0.0f && contact;
    t += ap.dt;
    air = (t - 0.5f) * (first ? 1.0f : 0.0f);
    v.feet_air_time[(size_t)4 * e + k] = t * (contact ? 0.0f : 1.0f);
  }
  tq2 = team16_sum(tq2);
  acc2 = team16_sum(acc2);
  rate2 = team16_sum(rate2);
  hip = team16_sum(hip);
  const float knees = team16_sum(knee);
  stumble = team16_sum(stumble);
  air = team16_sum(air);
  // ---- the root row: lane 0 of the team
  long long progress = 0;
  if (ok && tl == 0) {
    progress = (long long)tb.progress[e] + 1;
    float* r = st.root_states + (size_t)13 * e;
    if (v.push_now) {   // push_robots: the root tensor itself, so that the next simulate sees it
      r[7] = mgt::rand_float((float)(1.0 - -1.0), -1.0f, draw(tb, e, kColPush));
      r[8] = mgt::rand_float((float)(1.0 - -1.0), -1.0f, draw(tb, e, kColPush + 1));
    }
    float root[13];
#pragma unroll
    for (int c = 0; c < 13; c++) root[c] = r[c];
    const float grav[3] = {0.0f, 0.0f, -1.0f}, fwd[3] = {1.0f, 0.0f, 0.0f};
    float lin[3], ang[3], pg[3], f[3];
    mg::t_quat_rotate(root + 3, root + 7, lin, true);
    mg::t_quat_rotate(root + 3, root + 10, ang, true);
    mg::t_quat_rotate(root + 3, grav, pg, true);
    quat_apply(root + 3, fwd, f);
    const float heading = atan2f(f[1], f[0]);
    float* cm = v.commands + (size_t)4 * e;
    const float c0 = cm[0], c1 = cm[1], c3 = cm[3];
    float c2 = 0.5f * wrap_to_pi(c3 - heading);
    c2 = c2 < -1.0f ? -1.0f : (c2 > 1.0f ? 1.0f : c2);
    cm[2] = c2;
    s.cmd[g][0] = c0;
    s.cmd[g][1] = c1;
    s.cmd[g][2] = c2;
    s.cmd[g][3] = c3;
    // check_termination
    const float* bf = st.net_contact_forces + (size_t)3 * ((size_t)ap.num_bodies * e + ap.base_body);
    bool reset = norm3(bf) > 1.0f;
    if (!ap.allow_knee_contacts) reset = reset || knees > 0.0f;
    if (progress >= (long long)ap.max_episode_length - 1) reset = true;
    // compute_reward
    float* tm = s.term[g];
    const float d0 = c0 - lin[0], d1 = c1 - lin[1], d2 = c2 - ang[2];
    const float lin_err = d0 * d0 + d1 * d1, ang_err = d2 * d2;
    tm[0] = expf(-lin_err / 0.25f) * ap.rew_scale[0];
    tm[1] = (lin[2] * lin[2]) * ap.rew_scale[1];
    tm[2] = expf(-ang_err / 0.25f) * ap.rew_scale[2];
    tm[3] = (ang[0] * ang[0] + ang[1] * ang[1]) * ap.rew_scale[3];
    tm[4] = (pg[0] * pg[0] + pg[1] * pg[1]) * ap.rew_scale[4];
    tm[5] = tq2 * ap.rew_scale[5];
    tm[6] = acc2 * ap.rew_scale[6];
    const float dz = root[2] - 0.52f;
    tm[7] = (dz * dz) * ap.rew_scale[7];
    tm[8] = (air * ap.rew_scale[8]) * (sqrtf(c0 * c0 + c1 * c1) > 0.1f ? 1.0f : 0.0f);
    tm[9] = knees * ap.rew_scale[9];
    tm[10] = stumble * ap.rew_scale[10];
    tm[11] = rate2 * ap.rew_scale[11];
    tm[12] = hip * ap.rew_scale[12];
    // the reference's order of the sum (anymal_terrain.py:362-363)
    float rew = tm[0] + tm[2] + tm[1] + tm[3] + tm[4] + tm[7] + tm[5] + tm[6] + tm[9] + tm[11] + tm[8] + tm[12] + tm[10];
    rew = rew > 0.0f ? rew : 0.0f;
    // the termination reward: timeout_buf is the previous step's here
    rew += ap.rew_termination * ((reset && tb.timeout[e] == 0) ? 1.0f : 0.0f);
    s.rew[g] = rew;
    s.reset[g] = reset ? 1 : 0;
    float* o = s.obs + kObs * g;   // the base-frame columns: a reset below leaves them as they are
#pragma unroll
    for (int i = 0; i < 3; i++) {
      o[i] = lin[i] * ap.lin_vel_scale;
      o[3 + i] = ang[i] * ap.ang_vel_scale;
      o[6 + i] = pg[i];
      s.root[g][i] = root[i];
    }
#pragma unroll
    for (int c = 3; c < 13; c++) s.root[g][c] = root[c];
  }
  if (!ok && tl == 0) s.reset[g] = 0;
  __syncthreads();
  // ---- episode_sums += term, the 13 columns over the team's lanes; a reset env hands its sums over and starts at 0
  const bool do_reset = ok && s.reset[g] != 0;
  if (ok && tl < kRew) {
    float* es = v.episode_sums + (size_t)kRew * e + tl;
    const float sum = *es + s.term[g][tl];
    s.sums[g][tl] = sum;
    *es = do_reset ? 0.0f : sum;
  }
  // ---- reset_idx of the envs whose flag was just set
  reset_team(ap, v, tb, st, ee, tl, do_reset, true, s.root[g], s.cmd[g], pos, vel);
  if (ok && tl == kRew) s.sums[g][kRew] = do_reset ? 1.0f : 0.0f;
  if (ok && tl == kRew + 1) s.sums[g][kRew + 1] = (float)v.terrain_levels[e];   // the reset's update is behind a barrier
  if (ok && tl == kRew + 2) s.sums[g][kRew + 2] = 0.0f;
  // ---- observations: commands, DOF state, heights, actions
  float* o = s.obs + kObs * g;
  if (ok && tl < 3) o[9 + tl] = s.cmd[g][tl] * (tl < 2 ? ap.lin_vel_scale : ap.ang_vel_scale);
  if (ok && tl < kDofs) {
    const size_t i = (size_t)kDofs * e + tl;
    o[12 + tl] = pos * ap.dof_pos_scale;
    o[24 + tl] = vel * ap.dof_vel_scale;
    o[36 + kPts + tl] = act;
    v.last_actions[i] = act;    // for every env: the reset's zeroing is overwritten (anymal_terrain.py:484-485)
    v.last_dof_vel[i] = vel;
  }
  if (ok) {
    const float* r = s.root[g];
    for (int k = tl; k < kPts; k += kTeam) {
      const float h = ap.hf_heights ? scan_height(ap, r, ap.height_points[2 * k], ap.height_points[2 * k + 1]) : 0.0f;
      if (v.measured_heights) v.measured_heights[(size_t)kPts * e + k] = h;
      float x = r[2] - 0.5f - h;
      x = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
      o[36 + k] = x * ap.height_meas_scale;
    }
  }
  __syncthreads();
  if (ok && ap.add_noise) {
    for (int c = tl; c < kObs; c += kTeam) o[c] += (2.0f * draw(tb, e, kColObs + c) - 1.0f) * ap.noise_scale_vec[c];
  }
  // ---- the tail
  if (ok && tl == 0) {
    if (do_reset) progress = 0;
    mgt::tail_store(tb, e, s.rew[g], do_reset ? 1 : 0, progress, progress >= (long long)ap.max_episode_length - 1);
    s.rst[g] = do_reset ? 1.0f : 0.0f;
  }
  __syncthreads();
  const int first_env = blockIdx.x * kEnvs;
  const int rows = n_envs - first_env < kEnvs ? n_envs - first_env : kEnvs;
  store_partials(v, s, rows);
  mgt::block_tail(tb, s.obs, s.rew, s.rst, (size_t)first_env, rows, kObs, ap.clip_obs);
}

// The second stage of the means: one block of 256 lanes, lane (j, c) adds column c of the partial rows j, j + 16, ...
// in that order, lane (0, c) then adds the 16 segments in order.  episode_out = [13 means of the reset envs' sums /
// max_episode_length_s | mean terrain level of all envs], written only if some env reset.
__global__ __launch_bounds__(256) void k_at_finish(mg_anymal_terrain_params ap, mg_anymal_terrain_views v, int blocks,
                                                   int n_envs) {
  __shared__ float seg[16][kPart];
  const int c = threadIdx.x % kPart, j = threadIdx.x / kPart;
  float acc = 0.0f;
  for (int b = j; b < blocks; b += 16) acc += v.partials[(size_t)kPart * b + c];
  seg[j][c] = acc;
  __syncthreads();
  float tot = 0.0f;
  for (int k = 0; k < 16; k++) tot += seg[k][c];
  __syncthreads();
  if (j == 0) seg[0][c] = tot;
  __syncthreads();
  const float resets = seg[0][kRew];
  if (j != 0 || resets <= 0.0f) return;
  if (c < kRew) v.episode_out[c] = (tot / resets) / ap.max_episode_length_s;
  if (c == kRew) v.episode_out[kRew] = seg[0][kRew + 1] / (float)n_envs;
}

// reset_idx(env_ids), off the hot path, in two launches so that a repeated id meets no race: the listed envs are
// marked, then every marked env is reset once by its team
__global__ __launch_bounds__(256) void k_at_mark(int32_t* __restrict__ mark, const int32_t* __restrict__ ids, int n,
                                                 int n_envs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int e = ids[i];
  if (e >= 0 && e < n_envs) mark[e] = 1;
}

__global__ __launch_bounds__(64) void k_at_reset_marked(mg_anymal_terrain_params ap, mg_anymal_terrain_views v,
                                                        mg_task_buffers tb, State st, int update_levels, int n_envs) {
  __shared__ Shared s;
  const int lane = threadIdx.x, g = lane / kTeam, tl = lane % kTeam;
  const int e = blockIdx.x * kEnvs + g;
  const bool ok = e < n_envs;
  const int ee = ok ? e : 0;
  const bool on = ok && v.reset_mark[ee] != 0;
  if (tl == 0) s.reset[g] = on ? 1 : 0;
  if (on && tl < 13) s.root[g][tl] = st.root_states[(size_t)13 * e + tl];
  if (on && tl >= kDofs) s.cmd[g][tl - kDofs] = v.commands[(size_t)4 * e + (tl - kDofs)];
  __syncthreads();
  float pos = 0.0f, vel = 0.0f;
  reset_team(ap, v, tb, st, ee, tl, on, update_levels != 0, s.root[g], s.cmd[g], pos, vel);
  if (on && tl < kDofs) {
    v.last_actions[(size_t)kDofs * e + tl] = 0.0f;
    v.last_dof_vel[(size_t)kDofs * e + tl] = 0.0f;
  }
  if (ok && tl < kRew) {
    float* es = v.episode_sums + (size_t)kRew * e + tl;
    s.sums[g][tl] = *es;
    if (on) *es = 0.0f;
  }
  if (ok && tl == kRew) s.sums[g][kRew] = on ? 1.0f : 0.0f;
  if (ok && tl == kRew + 1) s.sums[g][kRew + 1] = (float)v.terrain_levels[e];
  if (ok && tl == kRew + 2) {
    s.sums[g][kRew + 2] = 0.0f;
    if (on) {
      tb.progress[e] = 0;
      tb.reset[e] = 1;   // anymal_terrain.py:418
      v.reset_mark[e] = 0;
    }
  }
  __syncthreads();
  const int first_env = blockIdx.x * kEnvs;
  store_partials(v, s, n_envs - first_env < kEnvs ? n_envs - first_env : kEnvs);
}

// the explicit PD torque of one decimation step: one lane per (env, DOF) element
__global__ __launch_bounds__(256) void k_at_pre(mg_anymal_terrain_params ap, const float* __restrict__ actions,
                                                float* __restrict__ actions_out, const float* __restrict__ dof_state,
                                                float* __restrict__ actuation, float* __restrict__ torques,
                                                long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float a = mg::clampf(actions[i], ap.clip_actions);
  if (actions_out) actions_out[i] = a;
  const float scaled = ap.action_scale * a;
  const float target = scaled + ap.default_dof_pos[(int)(i % kDofs)];
  const float err = target - dof_state[2 * i];
  const float p = ap.Kp * err;
  const float d = ap.Kd * dof_state[2 * i + 1];
  float t = p - d;
  t = t < -ap.torque_clip ? -ap.torque_clip : (t > ap.torque_clip ? ap.torque_clip : t);
  actuation[i] = t;
  torques[i] = t;
}

#pragma clang fp contract(fast)

}  // namespace mgat
