// migym.hip — C-ABI (include/migym.h) and kernels of the MI355X physics-step +
// observation/reward path.  One lane per actor/env; every kernel is
// asynchronous on the caller's stream; no entry point synchronises.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "dispatch.hpp"
#include "dynamics_tensors.hpp"
#include "render.hpp"
#include "anymal_task.hpp"  // as reach_task.hpp: restores FMA contraction at its end
#include "amp_task.hpp"     // likewise
#include "quadcopter_task.hpp"  // likewise
#include "reach_task.hpp"   // before hand_task.hpp: that header leaves FMA contraction off for the rest of this file
#include "hand_task.hpp"
#include "task.hpp"

namespace {
thread_local std::string g_err;
}  // namespace
int mgi::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
using mgi::fail;
using mgi::kBlock;
namespace {
int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MG_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
  return MG_OK;
}
inline int grid_for(int n) { return (n + kBlock - 1) / kBlock; }

// publish the phase-timing buffer to every instance's code object
template <int... I>
int publish_all(unsigned long long* buf, std::integer_sequence<int, I...>) {
  int rc = MG_OK;
  ((rc = rc ? rc : mgi::phase_buf_publish<I>(buf)), ...);
  return rc;
}
}  // namespace

__global__ __launch_bounds__(kBlock) void k_observations(mg_task_params tp, int n, const float* __restrict__ root,
                                                         const float* __restrict__ dof, const float* __restrict__ dforce,
                                                         const float* __restrict__ sensors,
                                                         const float* __restrict__ actions, float* pot, float* prev_pot,
                                                         float* up, float* heading, float* obs) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int nd = mg::t_dofs(&tp), ns = mg::t_sensors(&tp);
  const float zero3[3] = {0.0f, 0.0f, 0.0f};
  mg::obs_env(&tp, zero3, root + (size_t)13 * e, dof + (size_t)2 * nd * e, dforce ? dforce + (size_t)nd * e : nullptr,
              sensors ? sensors + (size_t)6 * ns * e : nullptr, actions + (size_t)tp.num_actions * e, pot + e,
              prev_pot + e, up + 3 * (size_t)e, heading + 3 * (size_t)e, obs + (size_t)tp.num_obs * e);
}

__global__ __launch_bounds__(kBlock) void k_reward(mg_task_params tp, int n, const float* __restrict__ obs,
                                                   const float* __restrict__ actions, const float* __restrict__ pot,
                                                   const float* __restrict__ prev_pot,
                                                   const int64_t* __restrict__ progress, int64_t* reset, float* rew) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  mg::reward_env(&tp, obs + (size_t)tp.num_obs * e, actions + (size_t)tp.num_actions * e, pot[e], prev_pot[e],
                 progress[e], reset + e, rew + e);
}

// post_physics_step + VecTask.step tail for actor a (state already advanced).  Multi-agent:
// actors of one env are adjacent lanes of one wave (64 % num_agents == 0), so the env-level
// AND of the agents' reset flags is a ballot and the other agents' torso positions are shuffles.
__device__ __forceinline__ void post_physics_env(const mg_task_params& tp, const mg_state_views& v,
                                                 const mg_task_buffers& tb, int a, const float* act,
                                                 int64_t reset_in) {
  const int nd = mg::t_dofs(&tp), ns = mg::t_sensors(&tp), no = tp.num_obs;
  const int A = tp.num_agents > 1 ? tp.num_agents : 1;
  const int k = a % A;
  const float* off = tp.agent_offset[k];
  float* root = v.root_states + (size_t)13 * a;
  float* dof = v.dof_state + (size_t)2 * nd * a;
  int64_t progress = tb.progress[a] + 1;
  int64_t reset = reset_in;
  bool do_reset = reset != 0;
  if (A > 1) {  // AND filter (franka_reach_MA.py:875-885)
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(reset != 0);
    const unsigned long long full = (A >= 64) ? ~0ull : ((1ull << A) - 1ull);
    do_reset = ((m >> (lane - k)) & full) == full;
  }
  float pot = tb.potentials ? tb.potentials[a] : 0.0f;
  float prev = tb.prev_potentials ? tb.prev_potentials[a] : 0.0f;
  if (do_reset) {
    mg::reset_env(&tp, off, tb.noise ? tb.noise + (size_t)2 * nd * a : nullptr, tb.seed,
                  (uint64_t)(tb.env_offset * A + a), tb.step_counter, root, dof, &pot, &prev);
    progress = 0;
    reset = 0;
  }
  float* o = tb.obs + (size_t)no * a;
  float up[3], hd[3];
  mg::obs_env(&tp, off, root, dof, v.dof_force ? v.dof_force + (size_t)nd * a : nullptr,
              v.sensors ? v.sensors + (size_t)6 * ns * a : nullptr, act, &pot, &prev, up, hd, o);
  if (A > 1) {  // "others" block: cyclic shift starting after self (franka_reach_MA.py:604-608)
    const int lane = threadIdx.x & 63;
    const float px = root[0], py = root[1], pz = root[2];
    const int base = no - 3 * (A - 1);
    for (int j = 1; j < A; j++) {
      const int src = lane - k + (k + j) % A;
      const float qx = __shfl(px, src), qy = __shfl(py, src), qz = __shfl(pz, src);
      o[base + 3 * (j - 1) + 0] = qx - px;
      o[base + 3 * (j - 1) + 1] = qy - py;
      o[base + 3 * (j - 1) + 2] = qz - pz;
    }
  }
  float rew;
  mg::reward_env(&tp, o, act, pot, prev, progress, &reset, &rew);
  const float max_ep_m1 = (float)tp.max_episode_length - 1.0f;
  tb.rew[a] = rew;
  tb.reset[a] = reset;
  tb.progress[a] = progress;
  tb.timeout[a] = (uint8_t)(((float)progress >= max_ep_m1) && (reset != 0));
  if (tp.task_id != MG_TASK_CARTPOLE) {
    tb.potentials[a] = pot;
    tb.prev_potentials[a] = prev;
    for (int c = 0; c < 3; c++) {
      tb.up_vec[3 * (size_t)a + c] = up[c];
      tb.heading_vec[3 * (size_t)a + c] = hd[c];
    }
  }
  if (tb.obs_clamped)
    for (int i = 0; i < no; i++) tb.obs_clamped[(size_t)no * a + i] = mg::clampf(o[i], tp.clip_obs);
  if (tb.out_pack) {  // the gather's message row [clamped obs | rew | reset]
    float* pk = tb.out_pack + (size_t)(no + 2) * a;
    for (int i = 0; i < no; i++) pk[i] = mg::clampf(o[i], tp.clip_obs);
    pk[no] = rew;
    pk[no + 1] = (float)reset;
  }
}

__global__ __launch_bounds__(kBlock) void k_post_physics(mg_task_params tp, mg_state_views v, mg_task_buffers tb,
                                                         int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int na = tp.num_actions;
  float act[64];
  for (int i = 0; i < na; i++) {
    act[i] = mg::clampf(tb.actions[(size_t)na * e + i], tp.clip_actions);
    if (tb.actions_out) tb.actions_out[(size_t)na * e + i] = act[i];
  }
  post_physics_env(tp, v, tb, e, act, tb.reset[e]);
}


// pre_physics_step of the locomotion tasks: effort = clamp(a) * gear * power_scale
// (ant.py:281-285, humanoid.py:281-285; cartpole.py:159-163: DOF 0 only)
__global__ __launch_bounds__(kBlock) void k_pre_loco(mg_task_params tp, mg_state_views v, mg_task_buffers tb, int n,
                                                     int nd) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * nd) return;
  const int a = t / nd, d = t % nd, na = tp.num_actions;
  float tau;
  if (tp.task_id == MG_TASK_CARTPOLE) {
    tau = d == 0 ? mg::clampf(tb.actions[(size_t)na * a], tp.clip_actions) * tp.power_scale : 0.0f;
  } else {
    const float act = d < na ? mg::clampf(tb.actions[(size_t)na * a + d], tp.clip_actions) : 0.0f;
    tau = act * tp.motor_effort[d] * tp.power_scale;
  }
  const_cast<float*>(v.dof_actuation)[t] = tau;
}


// reset_idx of one ShadowHand env on one lane (shadow_hand.py:586-668): goal (reset_target_pose), object
// pose, hand DOFs and PD targets, counters
__device__ void hand_reset_env(const mg_task_params& tp, const mg_state_views& v, const mg_task_buffers& tb, int e,
                               int nd, uint64_t gid) {
  float* root = v.root_states + (size_t)39 * e;
  float* gs = tb.goal_states + (size_t)13 * e;
  float* tgt = const_cast<float*>(v.dof_targets) + (size_t)nd * e;
  float* prev = tb.prev_targets + (size_t)nd * e;
  {
    mg::h_reset_goal(tp, mg::h_rand_pm1(mg::h_uniform(tb, e, gid, 57)),
                     mg::h_rand_pm1(mg::h_uniform(tb, e, gid, 58)), gs, root + 26);
    float r[5];
    for (int k = 0; k < 5; k++) r[k] = mg::h_rand_pm1(mg::h_uniform(tb, e, gid, 4 + k));
    float* ob = root + 13;
    for (int k = 0; k < 3; k++) ob[k] = tp.object_start[k] + tp.reset_position_noise * r[k];
    mg::h_object_reset_rotation(tp, r[3], r[4], ob + 3);
    for (int k = 7; k < 13; k++) ob[k] = 0.0f;
    float* dof = v.dof_state + (size_t)2 * nd * e;
    for (int j = 0; j < nd; j++) {
      const float rp = mg::h_rand_pm1(mg::h_uniform(tb, e, gid, 9 + j));
      const float rv = mg::h_rand_pm1(mg::h_uniform(tb, e, gid, 9 + nd + j));
      const float dmax = tp.dof_upper[j] - tp.initial_dof_pos[j], dmin = tp.dof_lower[j] - tp.initial_dof_pos[j];
      const float pos = tp.initial_dof_pos[j] + tp.reset_dof_pos_noise * (dmin + (dmax - dmin) * 0.5f * (rp + 1.0f));
      dof[2 * j] = pos;
      dof[2 * j + 1] = 0.0f + tp.reset_dof_vel_noise * rv;
      prev[j] = pos;
      tgt[j] = pos;
    }
    tb.progress[e] = 0;
    tb.reset[e] = 0;
    tb.successes[e] = 0.0f;
  }
}

// reset_idx(ids) of the locomotion tasks, one lane per listed actor (ant.py:252-279): DOF noise, root row
// and potentials from task.hpp's reset_dof / reset_root (the fused step's own reset code), counters cleared
__global__ __launch_bounds__(kBlock) void k_reset_idx(mg_task_params tp, mg_state_views v, mg_task_buffers tb,
                                                      const int32_t* ids, int n, int n_actors) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int a = ids[t];
  if (a < 0 || a >= n_actors) return;
  if (tp.task_id == MG_TASK_SHADOW_HAND) {
    const uint64_t gid = (uint64_t)(tb.env_offset + a);
    hand_reset_env(tp, v, tb, a, tp.num_dofs, gid);
    tb.reset_goal[a] = 0;
    // random object forces: reset_idx zeroes the force and redraws the env's probability (shadow_hand.py:641-643)
    if (tb.random_force_prob) {
      const float lhi = logf(tp.force_prob_hi);
      tb.random_force_prob[a] = expf((logf(tp.force_prob_lo) - lhi) * mg::h_uniform(tb, a, gid, mg::HN_FORCE_PROB) + lhi);
    }
    if (v.rb_forces)
      for (int k = 0; k < 3; k++) v.rb_forces[((size_t)tp.rb_per_env * a + tp.rb_per_env - 2) * 3 + k] = 0.0f;
    return;
  }
  const int A = tp.num_agents > 1 ? tp.num_agents : 1;
  const int nd = mg::t_dofs(&tp);
  const float* nz = tb.noise ? tb.noise + (size_t)2 * nd * a : nullptr;
  float* dof = v.dof_state + (size_t)2 * nd * a;
  for (int i = 0; i < nd; i++)
    mg::reset_dof(&tp, i, nd, nz, tb.seed, (uint64_t)(tb.env_offset * A + a), tb.step_counter, dof);
  float pot = 0.0f, prev = 0.0f;
  mg::reset_root(&tp, tp.agent_offset[a % A], v.root_states + (size_t)13 * a, &pot, &prev);
  if (tp.task_id != MG_TASK_CARTPOLE && tb.potentials) {
    tb.potentials[a] = pot;
    tb.prev_potentials[a] = prev;
  }
  tb.progress[a] = 0;
  tb.reset[a] = 0;
}

// pre_physics_step of one env on one lane (physics-free path, shadow_hand.py:670-698)
__global__ __launch_bounds__(kBlock) void k_hand_pre(mg_task_params tp, mg_state_views v, mg_task_buffers tb,
                                                     int n, int nd) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint64_t gid = (uint64_t)(tb.env_offset + e);
  float* root = v.root_states + (size_t)39 * e;
  float* gs = tb.goal_states + (size_t)13 * e;
  const bool goal_reset = tb.reset_goal[e] != 0, env_reset = tb.reset[e] != 0;
  if (goal_reset)
    mg::h_reset_goal(tp, mg::h_rand_pm1(mg::h_uniform(tb, e, gid, 0)), mg::h_rand_pm1(mg::h_uniform(tb, e, gid, 1)),
                     gs, root + 26);
  float* tgt = const_cast<float*>(v.dof_targets) + (size_t)nd * e;
  float* prev = tb.prev_targets + (size_t)nd * e;
  if (env_reset) hand_reset_env(tp, v, tb, e, nd, gid);
  if (goal_reset || env_reset) tb.reset_goal[e] = 0;
  const int na = tp.num_actions;
  for (int i = 0; i < na; i++) {
    const int d = tp.actuated_dof[i];
    const float a = mg::clampf(tb.actions[(size_t)na * e + i], tp.clip_actions);
    if (tb.actions_out) tb.actions_out[(size_t)na * e + i] = a;
    const float t = mg::h_target(tp, d, a, prev[d]);
    tgt[d] = t;
    prev[d] = t;
  }
  // random object forces (reset_idx's zeroing + probability redraw, then decay / new draws)
  if (v.rb_forces || tb.random_force_prob) {
    float* fr = v.rb_forces ? v.rb_forces + ((size_t)tp.rb_per_env * e + tp.object_rb) * 3 : nullptr;
    float f[3] = {fr ? fr[0] : 0.0f, fr ? fr[1] : 0.0f, fr ? fr[2] : 0.0f};
    mg::h_object_force(tp, tb, e, gid, env_reset, f);
    if (fr)
      for (int k = 0; k < 3; k++) fr[k] = f[k];
  }
}

// observation value k of one env from its state rows (observationType layout, hand_task.hpp)
__device__ __forceinline__ float hand_obs_value(int layout, const mg_task_params& tp, int k, int nd, const float* dof,
                                                const float* dforce, const float* orow, const float* gs,
                                                const float* qdiff, const float* rbs, const float* sens,
                                                const float* act) {
  int i;
  const int seg = mg::h_locate_in(layout, tp, nd, k, &i);
  if (seg == mg::HS_FT_STATE || seg == mg::HS_FT_POS) {
    int b, c;
    mg::h_ft_ref(tp, seg, i, &b, &c);
    return rbs[(size_t)13 * b + c];
  }
  return mg::h_obs_value(tp, seg, i, dof, dforce, orow, gs, qdiff, sens, act);
}

// post_physics_step of one env on one lane (physics-free path): progress, full_state obs, reward,
// the running-mean partial sums, timeout, obs clamp
__global__ __launch_bounds__(kBlock) void k_hand_post(mg_task_params tp, mg_state_views v, mg_task_buffers tb,
                                                      int n, int nd) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  int64_t ro = 0;
  float fin = 0.0f;
  if (e < n) {
    const int na = tp.num_actions, no = tp.num_obs;
    const float* orow = v.root_states + (size_t)39 * e + 13;
    const float* gs = tb.goal_states + (size_t)13 * e;
    const float* act = tb.actions_out + (size_t)na * e;
    float qdiff[4];
    const float gc[4] = {-gs[3], -gs[4], -gs[5], gs[6]};
    mg::t_quat_mul(orow + 3, gc, qdiff);
    int64_t prog = tb.progress[e] + 1;
    float* o = tb.obs + (size_t)no * e;
    const float* rbs = v.rigid_body_states + (size_t)13 * tp.rb_per_env * e;
    for (int k = 0; k < no; k++) {
      const float x = hand_obs_value(tp.obs_type, tp, k, nd, v.dof_state + (size_t)2 * nd * e,
                                     v.dof_force + (size_t)nd * e, orow, gs, qdiff, rbs,
                                     v.sensors + (size_t)6 * tp.num_fingertips * e, act);
      o[k] = x;
      if (tb.obs_clamped) tb.obs_clamped[(size_t)no * e + k] = mg::clampf(x, tp.clip_obs);
    }
    if (tb.states)  // asymmetric_observations: states_buf = compute_full_state(asymm_obs=True)
      for (int k = 0; k < tp.num_states; k++)
        tb.states[(size_t)tp.num_states * e + k] =
            hand_obs_value(0, tp, k, nd, v.dof_state + (size_t)2 * nd * e, v.dof_force + (size_t)nd * e, orow, gs,
                           qdiff, rbs, v.sensors + (size_t)6 * tp.num_fingertips * e, act);
    float succ = tb.successes[e], rew;
    int64_t go;
    mg::h_reward(tp, orow, orow + 3, gs, gs + 3, act, tb.reset[e], tb.reset_goal[e], &prog, &succ, &rew, &ro, &go);
    tb.rew[e] = rew;
    tb.reset[e] = ro;
    tb.reset_goal[e] = go;
    tb.progress[e] = prog;
    tb.successes[e] = succ;
    tb.timeout[e] = (uint8_t)((prog >= (int64_t)tp.max_episode_length - 1) && (ro != 0));
    fin = succ * (float)ro;
    if (tb.out_pack) {  // the gather's message row [clamped obs | rew | reset]
      float* pk = tb.out_pack + (size_t)(no + 2) * e;
      for (int k = 0; k < no; k++) pk[k] = mg::clampf(o[k], tp.clip_obs);
      pk[no] = rew;
      pk[no + 1] = (float)ro;
    }
  }
  // partial sums of compute_hand_reward's global reduction (integer-valued: exact in any order)
  unsigned long long cr = (unsigned long long)ro, cf = (unsigned long long)fin;
  for (int off = 32; off >= 1; off >>= 1) {
    cr += __shfl_xor(cr, off);
    cf += __shfl_xor(cf, off);
  }
  if ((threadIdx.x & 63) == 0 && (cr | cf)) {
    atomicAdd((unsigned long long*)&tb.reduce_scratch[0], cr);
    atomicAdd((unsigned long long*)&tb.reduce_scratch[1], cf);
  }
}

// consecutive_successes running mean (shadow_hand.py:795-798) from the step's sums; clears them
__global__ void k_hand_finalize(mg_task_params tp, mg_task_buffers tb) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t nres = (int64_t)tb.reduce_scratch[0];
  const float fin = (float)tb.reduce_scratch[1];
  tb.consecutive_successes[0] = mg::h_cons_update(tp, nres, fin, tb.consecutive_successes[0]);
  tb.reduce_scratch[0] = 0;
  tb.reduce_scratch[1] = 0;
}


__global__ void k_set_indexed(float* __restrict__ dst, const float* __restrict__ src, const int32_t* __restrict__ idx,
                              int nidx, int row, int div) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nidx * row) return;
  const int r = t / row, c = t % row;
  const size_t a = (size_t)(idx[r] / div) * row + c;
  dst[a] = src[a];
}

// ------------------------------------------------------------------------------------------------ domain randomization
// dr_utils.generate_random_samples: the schedule scaling, then one draw of the descriptor's distribution
// (gaussian: np.random.normal(mu, var) = mu + var z).  Double precision like the reference's numpy.
__device__ double dr_sched(const mg_dr_desc& d, int64_t last_step) {
  if (d.schedule == MG_DR_SCHED_LINEAR)
    return 1.0 / (double)d.schedule_steps * (double)(last_step < d.schedule_steps ? last_step : d.schedule_steps);
  if (d.schedule == MG_DR_SCHED_CONSTANT) return last_step < d.schedule_steps ? 0.0 : 1.0;
  return 1.0;
}
__device__ double dr_sample(const mg_dr_desc& d, double sc, float u1, float u2) {
  double a = d.range[0], b = d.range[1];
  if (d.distribution == MG_DR_GAUSSIAN) {
    if (d.operation == MG_DR_ADDITIVE) { a *= sc; b *= sc; }
    else { b = b * sc; a = a * sc + 1.0 * (1.0 - sc); }
    const double z = sqrt(-2.0 * log(1.0 - (double)u1)) * cos(6.283185307179586 * (double)u2);
    return a + b * z;
  }
  if (d.operation == MG_DR_ADDITIVE) { a *= sc; b *= sc; }
  else { a = a * sc + 1.0 * (1.0 - sc); b = b * sc + 1.0 * (1.0 - sc); }
  if (d.distribution == MG_DR_LOGUNIFORM) return exp(log(a) + (log(b) - log(a)) * (double)u1);
  return a + (b - a) * (double)u1;
}
// dr_utils.get_bucketed_val: floor onto num_buckets buckets of the unscheduled range (uniform: [lo, hi];
// otherwise [mu - 2 sqrt(var), mu + 2 sqrt(var)]); below the first bucket Python's index -1 wraps to the last
__device__ double dr_bucket(const mg_dr_desc& d, double v) {
  double lo, hi;
  if (d.distribution == MG_DR_UNIFORM) { lo = d.range[0]; hi = d.range[1]; }
  else { lo = d.range[0] - 2.0 * sqrt((double)d.range[1]); hi = d.range[0] + 2.0 * sqrt((double)d.range[1]); }
  const int nb = d.num_buckets;
  int cnt = 0;  // bisect_right
  for (int i = 0; i < nb; i++)
    if ((hi - lo) * (double)i / (double)nb + lo <= v) cnt = i + 1;
  const int idx = cnt - 1 < 0 ? nb - 1 : cnt - 1;
  return (hi - lo) * (double)idx / (double)nb + lo;
}

// apply_randomizations' actor-property part for one actor per thread (vec_task.py:626-637, 746-842): the
// actor is randomized on the first call, or when randomize_buf >= frequency on a resetting step (then its
// counter restarts); each attribute element gets op(og, sample) (+ buckets) in its env_props column.
// Properties holding a setup_only attribute are only randomized on the first call.
__global__ __launch_bounds__(kBlock) void k_dr_apply(mg_dr_apply_args a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  bool doit = a.first != 0;
  if (!doit) {
    int64_t rb = a.randomize_buf[e] + (a.increment ? 1 : 0);
    doit = rb >= (int64_t)a.frequency && a.reset_mask[e] != 0;
    if (doit) rb = 0;
    a.randomize_buf[e] = rb;
  }
  if (!doit) return;
  const uint64_t gid = (uint64_t)(a.env_offset + e);
  float* row = a.env_props + (size_t)a.stride * e;
  for (int i = 0; i < a.nattr; i++) {
    const mg_dr_attr at = a.attrs[i];
    const mg_dr_desc d = a.descs[at.desc];
    if (!a.first && !d.after_setup) continue;
    double smp;
    if (a.samples) {
      smp = (double)a.samples[(size_t)a.nattr * e + i];
    } else {
      const float u1 = mg::uniform01(a.seed, gid, a.counter, (uint32_t)(8192 + 2 * i));
      const float u2 = mg::uniform01(a.seed, gid, a.counter, (uint32_t)(8193 + 2 * i));
      smp = dr_sample(d, dr_sched(d, a.last_step), u1, u2);
    }
    double v = d.operation == MG_DR_SCALING ? (double)at.og * smp : (double)at.og + smp;
    if (d.num_buckets > 0) v = dr_bucket(d, v);
    row[at.slot] = (float)v;
  }
}

// noise_lambda (vec_task.py:684-720) over a flat tensor; corr is (re)drawn when refresh_corr is set
__global__ __launch_bounds__(kBlock) void k_dr_noise(mg_dr_noise_args a) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t gid = (uint64_t)(a.elem_offset + i);
    float c;
    if (a.refresh_corr) {
      if (a.injected_corr) {
        c = a.injected_corr[i];
      } else {
        const float u1 = mg::uniform01(a.seed, gid, a.counter, 4 * a.key), u2 = mg::uniform01(a.seed, gid, a.counter, 4 * a.key + 1);
        c = sqrtf(-2.0f * logf(1.0f - u1)) * cosf(6.28318530717958647f * u2);
      }
      a.corr[i] = c;
    } else {
      c = a.corr[i];
    }
    float z;
    if (a.injected) {
      z = a.injected[i];
    } else {
      const float u1 = mg::uniform01(a.seed, gid, a.counter, 4 * a.key + 2);
      if (a.distribution == MG_DR_GAUSSIAN) {
        const float u2 = mg::uniform01(a.seed, gid, a.counter, 4 * a.key + 3);
        z = sqrtf(-2.0f * logf(1.0f - u1)) * cosf(6.28318530717958647f * u2);
      } else {
        z = u1;
      }
    }
    const float cc = c * a.c_scale + a.c_shift;
    const float nz = (cc + z * a.scale) + a.shift;
    const float x = a.operation == MG_DR_SCALING ? a.x[i] * nz : a.x[i] + nz;
    a.x[i] = x;
    if (a.x_clamped) a.x_clamped[i] = fminf(fmaxf(x, -a.clip), a.clip);
  }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

const char* mg_last_error(void) { return g_err.c_str(); }
int mg_version(void) { return MG_VERSION; }
size_t mg_model_sizeof(void) { return sizeof(mg_model); }
size_t mg_task_params_sizeof(void) { return sizeof(mg_task_params); }
size_t mg_task_buffers_sizeof(void) { return sizeof(mg_task_buffers); }
size_t mg_sim_params_sizeof(void) { return sizeof(mg_sim_params); }
size_t mg_state_views_sizeof(void) { return sizeof(mg_state_views); }
size_t mg_dr_desc_sizeof(void) { return sizeof(mg_dr_desc); }
size_t mg_dr_apply_args_sizeof(void) { return sizeof(mg_dr_apply_args); }
size_t mg_dr_noise_args_sizeof(void) { return sizeof(mg_dr_noise_args); }

// Profiling aid: per-phase shader cycles summed over all waves (blocks < 65536) since the last reset (phase-timing
// build only; returns MG_EINVAL otherwise).  Phases: 0 FK, 1 ABA (+tendons), 2 collide (+object
// free step), 3 rows, 4 row Jacobians / W, 5 test solves, 6 PGS, 7 integrate, 8 outputs, 9 task layer +
// write-back, 13 constraint rows (count), 14 load + pre-physics, 15 substep entry.
#ifdef MG_PHASE_TIMING
static unsigned long long* g_phase_host_buf = nullptr;  // the per-wave rows (kPhaseCap x MG_NUM_PHASES)
#endif

int mg_debug_phase_cycles(uint64_t* out, int32_t reset) {
#ifdef MG_PHASE_TIMING
  constexpr int kPhaseCap = 1 << 16;  // blocks tracked (step_kernels.hpp)
  unsigned long long*& buf = g_phase_host_buf;
  const size_t bytes = (size_t)kPhaseCap * MG_NUM_PHASES * sizeof(unsigned long long);
  if (!buf) {  // first call: allocate + zero the per-wave rows and publish them to the kernels
    if (hipMalloc(&buf, bytes) != hipSuccess || hipMemset(buf, 0, bytes) != hipSuccess)
      return fail(MG_EDEVICE, "mg_debug_phase_cycles: buffer setup failed");
    if (int rc = publish_all(buf, std::make_integer_sequence<int, MG_NUM_INST>{})) return rc;
    if (hipDeviceSynchronize() != hipSuccess) return fail(MG_EDEVICE, "mg_debug_phase_cycles: sync failed");
    if (out) memset(out, 0, MG_NUM_PHASES * sizeof(uint64_t));
    return MG_OK;
  }
  if (hipDeviceSynchronize() != hipSuccess) return fail(MG_EDEVICE, "mg_debug_phase_cycles: sync failed");
  if (out) {
    std::vector<unsigned long long> h((size_t)kPhaseCap * MG_NUM_PHASES);
    if (hipMemcpy(h.data(), buf, bytes, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(MG_EDEVICE, "mg_debug_phase_cycles: copy failed");
    for (int i = 0; i < MG_NUM_PHASES; i++) out[i] = 0;
    for (size_t w = 0; w < (size_t)kPhaseCap; w++)
      for (int i = 0; i < MG_NUM_PHASES; i++) out[i] += h[MG_NUM_PHASES * w + i];
  }
  if (reset && hipMemset(buf, 0, bytes) != hipSuccess) return fail(MG_EDEVICE, "mg_debug_phase_cycles: reset failed");
  if (hipDeviceSynchronize() != hipSuccess) return fail(MG_EDEVICE, "mg_debug_phase_cycles: sync failed");
  return MG_OK;
#else
  (void)out;
  (void)reset;
  return fail(MG_EINVAL, "mg_debug_phase_cycles: library built without MG_PHASE_TIMING");
#endif
}

// Profiling aid: the per-item rows behind mg_debug_phase_cycles (an item = one wave's 64 / T teams; rows of
// MG_NUM_PHASES cycle counts, summed since the last reset), the first `cap` items.  Phase-timing build only.
int mg_debug_phase_waves(uint64_t* out, int32_t cap) {
#ifdef MG_PHASE_TIMING
  constexpr int kPhaseCap = 1 << 16;
  if (!out || cap < 0 || cap > kPhaseCap) return fail(MG_EINVAL, "mg_debug_phase_waves: bad arguments");
  if (!g_phase_host_buf) return fail(MG_EINVAL, "mg_debug_phase_waves: call mg_debug_phase_cycles first");
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(out, g_phase_host_buf, (size_t)cap * MG_NUM_PHASES * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(MG_EDEVICE, "mg_debug_phase_waves: copy failed");
  return MG_OK;
#else
  (void)out;
  (void)cap;
  return fail(MG_EINVAL, "mg_debug_phase_waves: library built without MG_PHASE_TIMING");
#endif
}

int mg_sim_create(const mg_model* model, const mg_sim_params* params, int32_t num_envs, int32_t device,
                  mg_sim** out) {
  if (!model || !params || !out || num_envs <= 0) return fail(MG_EINVAL, "mg_sim_create: bad arguments");
  if (model->num_nodes < 1 || model->num_nodes > MG_MAX_NODES || model->num_geoms > MG_MAX_GEOMS ||
      model->num_pairs > MG_MAX_PAIRS || model->num_sensors > MG_MAX_SENSORS || model->num_bodies > MG_MAX_BODIES)
    return fail(MG_EINVAL, "mg_sim_create: model tables out of range");
  for (int i = 1; i < model->num_nodes; i++)
    if (model->parent[i] < 0 || model->parent[i] >= i)
      return fail(MG_EINVAL, "mg_sim_create: nodes must be topologically ordered (parent < child)");
  if (params->substeps < 1 || params->dt <= 0.0f || params->max_contacts < 0)
    return fail(MG_EINVAL, "mg_sim_create: bad sim params");
  if ((params->solver_type != MG_SOLVER_PGS && params->solver_type != MG_SOLVER_TGS) || params->vel_iters < 0)
    return fail(MG_EINVAL, "mg_sim_create: solver_type must be MG_SOLVER_PGS or MG_SOLVER_TGS, vel_iters >= 0");
  // the exact hull-object candidates are computed before the tree phases (team_physics.hpp hull_stage), from
  // the fixed root's pose: a convex-mesh geom colliding with a block / pen object must sit on that root
  if (model->obj_type == MG_GT_BOX || model->obj_type == MG_GT_CAPSULE)
    for (int g = 0; g < model->num_geoms; g++)
      if (model->geom_type[g] == MG_GT_CONVEX && (model->geom_filter[g] & MG_COLLIDE_OBJECT) &&
          (model->geom_node[g] != 0 || !model->fixed_base))
        return fail(MG_EINVAL, "mg_sim_create: a convex-mesh geom against the object must be on the fixed root");
  {  // one convex-mesh geom may collide with the object: the LDS tile stages one hull (build_tile's hullg)
    int ncvx = 0;
    for (int g = 0; g < model->num_geoms; g++)
      ncvx += model->geom_type[g] == MG_GT_CONVEX && (model->geom_filter[g] & MG_COLLIDE_OBJECT);
    if (model->obj_type && ncvx > 1)
      return fail(MG_EINVAL, "mg_sim_create: at most one convex-mesh geom may collide with the object");
  }
  if (hipSetDevice(device) != hipSuccess) return fail(MG_EDEVICE, "mg_sim_create: hipSetDevice failed");
  mg_sim* s = new (std::nothrow) mg_sim();
  if (!s) return fail(MG_ENOMEM, "mg_sim_create: out of host memory");
  s->host_model = *model;
  s->params = *params;
  s->n = num_envs;
  s->device = device;
  s->bound = false;
  s->link_forces = false;
  s->has_hf = false;
  s->hf = mg_heightfield{};
  if (hipMalloc(&s->d_model, sizeof(mg_model)) != hipSuccess) {
    delete s;
    return fail(MG_ENOMEM, "mg_sim_create: hipMalloc(model) failed");
  }
  if (hipMemcpy(s->d_model, model, sizeof(mg_model), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(s->d_model);
    delete s;
    return fail(MG_EDEVICE, "mg_sim_create: model upload failed");
  }
  // the LDS model tile of the instance that will run this model, prebuilt once on the host; a model no
  // instance fits is still created (its launches report MG_ECAPACITY)
  s->d_tile = nullptr;
  // work ordering (MgOrder, step_kernels.hpp: the envs in descending order of their last row counts)
  s->order_mode = kOrderOff;
  s->order_steps = 0;
  s->sort_every = 1;
  s->order_valid = false;
  s->d_bq = nullptr;
  s->d_blist = nullptr;
  s->bq_cap = 0;
  s->order_unit = s->order_agents = 1;
  s->d_order = nullptr;
  s->d_cost = nullptr;
  s->d_osort = nullptr;
  s->d_span = nullptr;
  s->span_cap = s->span_next = s->span_stride = 0;
  // default (same box, M env-steps/s unordered -> ordered): the sort for ShadowHand and Humanoid from
  // 16,384 envs and for Ant from 16,384 one-agent envs (ShadowHand 16,384 18.9 -> 20.1, in-kernel lists 20.0;
  // Humanoid 32,768 33.9 -> 37.3, lists 37.0; Ant 65,536 152.7 -> 157.8, lists 119.4: their hot-bucket atomics;
  // Ant 16,384: within noise under the last substep's row count as the key, 138.0 -> 148.4 under round 8's key counted
  // from the state the step leaves behind, profiles/r08/ab_zero_rows.txt);
  // off for MA-Ant (8,192 -0.8 %, 65,536 -1.0 % sorted; 8,192 +0.8 % under the round-8 key, inside three spreads),
  // Cartpole and the smaller batches (ShadowHand 4,096 -2 %: the sort's two launches outweigh the tail they save).
  // MIGYM_ORDER = off | lists | sort | sort:K (sort every K-th launch only; A/B: the order goes stale within two
  // steps) overrides.
  {
    const int T = mgi::team_size(s->host_model, s->params.max_contacts);
    const int A = params->agents > 1 ? params->agents : 1;
    if (T >= 32) s->order_mode = num_envs >= 16384 ? kOrderSort : kOrderOff;
    else if (T == 16 && A == 1) s->order_mode = num_envs >= 16384 ? kOrderSort : kOrderOff;
  }
  s->lds_pad = 0;
  if (const char* e = getenv("MIGYM_LDS_PAD")) s->lds_pad = atoi(e) > 0 ? atoi(e) : 0;
  // team LDS layout: by default the classic layout for a batch the classic kernel holds resident
  // (dispatch.hpp kCompactMinWaves) and the compact 12-wave layout above it.  The two layouts round differently, so
  // a shard is the bit-identical slice of a bigger rollout only when both pick the same layout:
  // MIGYM_LAYOUT = compact | classic pins it (auto: the default).
  s->layout_n = s->n;
  if (const char* e = getenv("MIGYM_LAYOUT")) {
    if (!strcmp(e, "classic")) s->layout_n = 0;
    else if (!strcmp(e, "compact")) s->layout_n = kLayoutCompact;
    else if (strcmp(e, "auto")) {
      mg_sim_destroy(s);
      return fail(MG_EINVAL, "mg_sim_create: MIGYM_LAYOUT must be auto, compact or classic");
    }
  }
  if (const char* e = getenv("MIGYM_ORDER")) {
    if (!strcmp(e, "off")) s->order_mode = kOrderOff;
    else if (!strcmp(e, "lists")) s->order_mode = kOrderLists;
    else if (!strcmp(e, "sort")) s->order_mode = kOrderSort;
    else if (!strncmp(e, "sort:", 5) && atoi(e + 5) > 0) {
      s->order_mode = kOrderSort;
      s->sort_every = atoi(e + 5);
    } else {
      mg_sim_destroy(s);
      return fail(MG_EINVAL, "mg_sim_create: MIGYM_ORDER must be off, lists, sort or sort:K (K > 0)");
    }
  }
  if (s->order_mode != kOrderOff) {
    const int A = params->agents > 1 ? params->agents : 1;
    s->order_agents = A;
    s->order_unit = A;
    s->bq_cap = (num_envs + s->order_unit - 1) / s->order_unit;
    const size_t nu = (size_t)s->bq_cap, nb = (nu + 255) / 256;
    const bool ok = s->order_mode == kOrderLists
        ? hipMalloc(&s->d_bq, sizeof(unsigned) * (2 * kOrderBuckets + 1)) == hipSuccess &&
              hipMemset(s->d_bq, 0, sizeof(unsigned) * (2 * kOrderBuckets + 1)) == hipSuccess &&
              hipMalloc(&s->d_blist, sizeof(int) * 2 * (size_t)kOrderBuckets * nu) == hipSuccess
        : hipMalloc(&s->d_osort, sizeof(unsigned) * (kSortTot + 256 * nb) + sizeof(unsigned short) * (nu + 2)) == hipSuccess &&
              hipMemset(s->d_osort, 0, sizeof(unsigned) * kSortTot) == hipSuccess &&
              hipMalloc(&s->d_order, sizeof(int) * nu) == hipSuccess &&
              hipMalloc(&s->d_cost, nu) == hipSuccess && hipMemset(s->d_cost, 0, nu) == hipSuccess;
    if (!ok) {
      mg_sim_destroy(s);
      return fail(MG_ENOMEM, "mg_sim_create: hipMalloc(work order) failed");
    }
  }
  // the step kernels' work-queue counters: zero here, and zeroed again by the last wave of every launch
  if (hipMalloc(&s->d_wq, 2 * sizeof(unsigned)) != hipSuccess || hipMemset(s->d_wq, 0, 2 * sizeof(unsigned)) != hipSuccess) {
    mg_sim_destroy(s);
    return fail(MG_ENOMEM, "mg_sim_create: hipMalloc(work queue) failed");
  }
  // the dynamics-tensor kernels' model (mg_dynamics_refresh, mg_osc_torques): fixed-base articulations only
  s->d_dyn = nullptr;
  s->dyn = mg_dynamics_views{nullptr, nullptr};
  if (model->fixed_base && model->num_nodes >= 2) {
    bool ok = true;
    for (int b = 0; b < model->num_bodies; b++)
      ok = ok && model->body_node[b] >= 0 && model->body_node[b] < model->num_nodes;
    mgd::DynModel dm;
    mgd::build_dyn_model(*model, &dm);
    if (ok && (hipMalloc(&s->d_dyn, sizeof(dm)) != hipSuccess ||
               hipMemcpy(s->d_dyn, &dm, sizeof(dm), hipMemcpyHostToDevice) != hipSuccess)) {
      mg_sim_destroy(s);
      return fail(MG_ENOMEM, "mg_sim_create: hipMalloc(dynamics model) failed");
    }
  }
  if (mgi::team_size(s->host_model, s->params.max_contacts) > 0) {
    const int rc = mgi::dispatch<mgi::BuildTile>(s->host_model, s->params.max_contacts, s->layout_n, s);
    if (rc) {
      mg_sim_destroy(s);
      return rc;
    }
  }
  *out = s;
  return MG_OK;
}

int mg_sim_bind(mg_sim* sim, const mg_state_views* views) {
  if (!sim || !views || !views->root_states || !views->dof_state) return fail(MG_EINVAL, "mg_sim_bind: bad views");
  if (sim->host_model.num_sensors > 0 && !views->sensors)
    return fail(MG_EINVAL, "mg_sim_bind: model has force sensors but no sensor buffer");
  if (views->env_props && views->env_props_stride < mg_env_props_layout(&sim->host_model, nullptr))
    return fail(MG_EINVAL, "mg_sim_bind: env_props_stride is shorter than mg_env_props_layout's row");
  sim->views = *views;
  sim->bound = true;
  return MG_OK;
}

// what a launch on the sim's heightfield refuses (nothing launched or written)
static int heightfield_ok(const mg_sim* sim, const char* who) {
  if (sim->host_model.obj_type)
    return fail(MG_EINVAL, std::string(who) + ": a heightfield has no instance for a model with a free object");
  if (sim->views.env_props)
    return fail(MG_EINVAL, std::string(who) + ": a heightfield has no domain-randomized instance (env_props is bound)");
  if (sim->layout_n >= kLayoutCompact)
    return fail(MG_EINVAL, std::string(who) + ": a heightfield has no instance in the compact layout (MIGYM_LAYOUT=compact)");
  if (sim->link_forces)
    return fail(MG_EINVAL, std::string(who) + ": a heightfield has no instance with link forces (mg_sim_set_link_forces is on)");
  return MG_OK;
}

int mg_sim_simulate(mg_sim* sim, void* stream) {
  if (!sim || !sim->bound) return fail(MG_EINVAL, "mg_sim_simulate: sim not bound");
  if (sim->has_hf) {
    // heightfield terrain (mg_sim_set_heightfield): the classic layout's own instances at every batch size
    if (int rc = heightfield_ok(sim, "mg_sim_simulate")) return rc;
    int rc = mgi::dispatch<mgi::SimulateHF>(sim->host_model, sim->params.max_contacts, 0L, (hipStream_t)stream,
                                            (const mg_sim*)sim);
    if (rc) return rc;
    return check_launch("mg_sim_simulate");
  }
  if (sim->link_forces) {
    // link forces (mg_sim_set_link_forces): the classic layout's own instances at every batch size
    if (!sim->views.rb_forces) return fail(MG_EINVAL, "mg_sim_simulate: link forces are on and no rb_forces tensor is bound");
    if (sim->views.env_props)
      return fail(MG_EINVAL, "mg_sim_simulate: link forces have no domain-randomized instance (env_props is bound)");
    if (sim->layout_n >= kLayoutCompact)
      return fail(MG_EINVAL, "mg_sim_simulate: link forces have no instance in the compact layout (MIGYM_LAYOUT=compact)");
    int rc = mgi::dispatch<mgi::SimulateXF>(sim->host_model, sim->params.max_contacts, 0L, (hipStream_t)stream,
                                            (const mg_sim*)sim);
    if (rc) return rc;
    return check_launch("mg_sim_simulate");
  }
  int rc = mgi::dispatch<mgi::RunSimulate>(sim->host_model, sim->params.max_contacts, sim->layout_n, (hipStream_t)stream,
                                 (const mg_sim*)sim);
  if (rc) return rc;
  return check_launch("mg_sim_simulate");
}

// the field's own checks (they need no sim, and come first)
static int heightfield_args_ok(const mg_heightfield* hf) {
  if (!hf->heights) return fail(MG_EINVAL, "mg_sim_set_heightfield: heights is NULL");
  if (hf->nx < 2 || hf->ny < 2) return fail(MG_EINVAL, "mg_sim_set_heightfield: nx and ny must be at least 2");
  if (!std::isfinite(hf->dx) || !(hf->dx > 0.0f))
    return fail(MG_EINVAL, "mg_sim_set_heightfield: dx must be finite and positive");
  if (!std::isfinite(hf->x0) || !std::isfinite(hf->y0) || !std::isfinite(hf->hmax))
    return fail(MG_EINVAL, "mg_sim_set_heightfield: x0, y0 and hmax must be finite");
  return MG_OK;
}

int mg_sim_set_heightfield(mg_sim* sim, const mg_heightfield* hf) {
  if (hf)
    if (int rc = heightfield_args_ok(hf)) return rc;
  if (!sim) return fail(MG_EINVAL, "mg_sim_set_heightfield: bad arguments (sim is NULL)");
  sim->has_hf = hf != nullptr;   // NULL: back to the plane z = 0
  sim->hf = hf ? *hf : mg_heightfield{};
  return MG_OK;
}

size_t mg_heightfield_sizeof(void) { return sizeof(mg_heightfield); }

int mg_height_scan(mg_sim* sim, const float* points, int32_t num_points, float* out, void* stream) {
  if (!sim || !sim->bound) return fail(MG_EINVAL, "mg_height_scan: sim not bound");
  if (!sim->has_hf) return fail(MG_EINVAL, "mg_height_scan: no heightfield is set (mg_sim_set_heightfield)");
  if (!points || !out || num_points < 0) return fail(MG_EINVAL, "mg_height_scan: bad arguments");
  if (sim->host_model.obj_type)
    return fail(MG_EINVAL, "mg_height_scan: a heightfield has no instance for a model with a free object");
  if (!sim->views.root_states) return fail(MG_EINVAL, "mg_height_scan: needs root_states");
  if (sim->n == 0 || num_points == 0) return MG_OK;
  mgi::launch_height_scan((hipStream_t)stream, sim, points, num_points, out);
  return check_launch("mg_height_scan");
}

int mg_sim_set_link_forces(mg_sim* sim, int32_t enable) {
  if (!sim) return fail(MG_EINVAL, "mg_sim_set_link_forces: bad arguments");
  sim->link_forces = enable != 0;
  return MG_OK;
}

// Tests only: the contact list the first substep of mg_sim_simulate would build from the bound state (k_contacts,
// the instance and layout mg_sim_simulate's dispatch picks); the DR and TGS instances have no read-out
int mg_debug_contacts(mg_sim* sim, float* out, int32_t* count, int32_t cap, void* stream) {
  if (!sim || !sim->bound) return fail(MG_EINVAL, "mg_debug_contacts: sim not bound");
  if (!out || !count || cap < 0) return fail(MG_EINVAL, "mg_debug_contacts: bad arguments");
  if (sim->views.env_props || sim->params.solver_type != MG_SOLVER_PGS)
    return fail(MG_EINVAL, "mg_debug_contacts: no read-out of the domain-randomized or TGS instances");
  if (sim->has_hf) {
    if (int rc = heightfield_ok(sim, "mg_debug_contacts")) return rc;
    int rc = mgi::dispatch<mgi::ContactsHF>(sim->host_model, sim->params.max_contacts, 0L, (hipStream_t)stream,
                                            (const mg_sim*)sim, out, count, cap);
    if (rc) return rc;
    return check_launch("mg_debug_contacts");
  }
  int rc = mgi::dispatch<mgi::RunContacts>(sim->host_model, sim->params.max_contacts, sim->layout_n, (hipStream_t)stream,
                                           (const mg_sim*)sim, out, count, cap);
  if (rc) return rc;
  return check_launch("mg_debug_contacts");
}

int mg_sim_set_params(mg_sim* sim, const mg_sim_params* params) {
  if (!sim || !params || params->substeps < 1 || params->dt <= 0.0f || params->max_contacts < 0)
    return fail(MG_EINVAL, "mg_sim_set_params: bad arguments");
  if (params->max_contacts != sim->params.max_contacts || params->agents != sim->params.agents)
    return fail(MG_EINVAL, "mg_sim_set_params: max_contacts / agents are fixed at mg_sim_create");
  if ((params->solver_type != MG_SOLVER_PGS && params->solver_type != MG_SOLVER_TGS) || params->vel_iters < 0)
    return fail(MG_EINVAL, "mg_sim_set_params: solver_type must be MG_SOLVER_PGS or MG_SOLVER_TGS, vel_iters >= 0");
  sim->params = *params;  // taken by value by every later launch
  return MG_OK;
}

int mg_env_props_layout(const mg_model* m, int32_t offsets[4]) {
  if (!m) return fail(MG_EINVAL, "mg_env_props_layout: bad model");
  const int o0 = 0, o1 = MG_EP_NODE_WIDTH * m->num_nodes, o2 = o1 + m->num_geoms, o3 = o2 + 2 * m->num_tendons;
  if (offsets) { offsets[0] = o0; offsets[1] = o1; offsets[2] = o2; offsets[3] = o3; }
  return (o3 + 4 + 3) & ~3;
}

int mg_env_props_defaults(const mg_model* m, float* row) {
  if (!m || !row) return fail(MG_EINVAL, "mg_env_props_defaults: bad arguments");
  int32_t off[4];
  const int stride = mg_env_props_layout(m, off);
  for (int k = 0; k < stride; k++) row[k] = 0.0f;
  for (int i = 0; i < m->num_nodes; i++) {
    float* r = row + off[MG_EP_NODE] + MG_EP_NODE_WIDTH * i;
    r[0] = m->mass[i]; r[1] = m->armature[i]; r[2] = m->damping[i]; r[3] = m->stiffness[i];
    r[4] = m->lower[i]; r[5] = m->upper[i]; r[6] = m->drive_kp[i]; r[7] = m->effort_limit[i];
    r[8] = m->frictionloss[i];
  }
  for (int g = 0; g < m->num_geoms; g++) row[off[MG_EP_GEOM] + g] = 1.0f;  // shape friction (build-defined default)
  for (int q = 0; q < m->num_tendons; q++) {
    row[off[MG_EP_TENDON] + 2 * q] = m->tendon_limit_stiffness[q];
    row[off[MG_EP_TENDON] + 2 * q + 1] = m->tendon_damping[q];
  }
  float* o = row + off[MG_EP_OBJECT];
  o[0] = m->obj_mass; o[1] = 1.0f; o[2] = 1.0f; o[3] = 0.0f;
  return MG_OK;
}

int mg_dr_apply(const mg_dr_apply_args* a, void* stream) {
  if (!a || a->n < 0 || a->nattr < 0 || (a->nattr > 0 && (!a->descs || !a->attrs)) || !a->env_props ||
      a->stride <= 0 || (!a->first && (!a->reset_mask || !a->randomize_buf)))
    return fail(MG_EINVAL, "mg_dr_apply: bad arguments");
  if (a->n == 0) return MG_OK;
  hipLaunchKernelGGL(k_dr_apply, dim3(grid_for(a->n)), dim3(kBlock), 0, (hipStream_t)stream, *a);
  return check_launch("mg_dr_apply");
}

int mg_dr_noise(const mg_dr_noise_args* a, void* stream) {
  if (!a || !a->x || !a->corr || a->n < 0) return fail(MG_EINVAL, "mg_dr_noise: bad arguments");
  if (a->n == 0) return MG_OK;
  const int64_t blocks = (a->n + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_dr_noise, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kBlock), 0,
                     (hipStream_t)stream, *a);
  return check_launch("mg_dr_noise");
}

int mg_sim_destroy(mg_sim* sim) {
  if (!sim) return MG_OK;
  if (sim->d_model) (void)hipFree(sim->d_model);
  if (sim->d_tile) (void)hipFree(sim->d_tile);
  if (sim->d_wq) (void)hipFree(sim->d_wq);
  if (sim->d_bq) (void)hipFree(sim->d_bq);
  if (sim->d_blist) (void)hipFree(sim->d_blist);
  if (sim->d_order) (void)hipFree(sim->d_order);
  if (sim->d_cost) (void)hipFree(sim->d_cost);
  if (sim->d_osort) (void)hipFree(sim->d_osort);
  if (sim->d_span) (void)hipFree(sim->d_span);
  if (sim->d_dyn) (void)hipFree(sim->d_dyn);
  delete sim;
  return MG_OK;
}

int mg_kernel_span_begin(mg_sim* sim, int32_t cap) {
  if (!sim || cap < 0 || cap > (int32_t)(sizeof(sim->span_waves) / sizeof(sim->span_waves[0])))
    return fail(MG_EINVAL, "mg_kernel_span_begin: bad arguments (cap 0..1024)");
  if (sim->d_span) (void)hipFree(sim->d_span);
  sim->d_span = nullptr;
  sim->span_cap = sim->span_next = 0;
  if (cap == 0) return MG_OK;
  // a launch's waves: one per 64 / T actors (T = the instance's team size), rounded up to whole blocks (<= 8 waves)
  const int T = mgi::team_size(sim->host_model, sim->params.max_contacts);
  sim->span_stride = (int)(((int64_t)sim->n * (T > 0 ? T : 64) + 63) / 64) + 8;
  const size_t bytes = sizeof(unsigned long long) * 2 * (size_t)sim->span_stride * (size_t)cap;
  if (hipMalloc(&sim->d_span, bytes) != hipSuccess) {
    sim->d_span = nullptr;
    return fail(MG_ENOMEM, "mg_kernel_span_begin: hipMalloc failed");
  }
  // zeros: a launch that records nothing (a build without the hooks) reads back as a zero span
  if (hipMemset(sim->d_span, 0, bytes) != hipSuccess) return fail(MG_EDEVICE, "mg_kernel_span_begin: memset failed");
  sim->span_cap = cap;
  return MG_OK;
}

int mg_kernel_span_read(mg_sim* sim, double* ms, int32_t cap, int32_t* n_out) {
  if (!sim || !ms || !n_out || cap < 0) return fail(MG_EINVAL, "mg_kernel_span_read: bad arguments");
  *n_out = 0;
  const int n = sim->span_next < cap ? sim->span_next : cap;
  if (!sim->d_span || n == 0) return MG_OK;
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, sim->device) != hipSuccess || khz <= 0)
    return fail(MG_EDEVICE, "mg_kernel_span_read: wall clock rate query failed");
  if (hipDeviceSynchronize() != hipSuccess) return fail(MG_EDEVICE, "mg_kernel_span_read: sync failed");
  std::vector<unsigned long long> h;
  for (int i = 0; i < n; i++) {
    const int w = sim->span_waves[i];
    h.resize(2 * (size_t)w);
    if (hipMemcpy(h.data(), sim->d_span + 2 * (size_t)sim->span_stride * i, h.size() * sizeof(unsigned long long),
                  hipMemcpyDeviceToHost) != hipSuccess)
      return fail(MG_EDEVICE, "mg_kernel_span_read: copy failed");
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int k = 0; k < w; k++) {
      t0 = h[2 * k] < t0 ? h[2 * k] : t0;
      t1 = h[2 * k + 1] > t1 ? h[2 * k + 1] : t1;
    }
    ms[i] = t1 >= t0 ? (double)(t1 - t0) / (double)khz : -1.0;
  }
  *n_out = n;
  return MG_OK;
}

int mg_kernel_span_waves(mg_sim* sim, int32_t launch, uint64_t* out, int32_t cap, int32_t* n_out) {
  if (!sim || !out || !n_out || cap < 0 || launch < 0) return fail(MG_EINVAL, "mg_kernel_span_waves: bad arguments");
  *n_out = 0;
  if (!sim->d_span || launch >= sim->span_next) return MG_OK;
  const int w = sim->span_waves[launch] < cap ? sim->span_waves[launch] : cap;
  if (hipDeviceSynchronize() != hipSuccess) return fail(MG_EDEVICE, "mg_kernel_span_waves: sync failed");
  if (w > 0 && hipMemcpy(out, sim->d_span + 2 * (size_t)sim->span_stride * launch, 2 * (size_t)w * sizeof(uint64_t),
                         hipMemcpyDeviceToHost) != hipSuccess)
    return fail(MG_EDEVICE, "mg_kernel_span_waves: copy failed");
  *n_out = w;
  return MG_OK;
}

int mg_work_order(mg_sim* sim, int32_t* order, uint8_t* cost, int32_t cap, int32_t* mode, int32_t* n_out) {
  if (!sim || !mode || !n_out || cap < 0) return fail(MG_EINVAL, "mg_work_order: bad arguments");
  *mode = sim->order_mode;
  *n_out = 0;
  if (sim->order_mode != kOrderSort) return MG_OK;
  const int n = sim->bq_cap < cap ? sim->bq_cap : cap;
  if (hipDeviceSynchronize() != hipSuccess) return fail(MG_EDEVICE, "mg_work_order: sync failed");
  if (order) {
    if (sim->order_valid && sim->order_steps > 1) {
      if (n > 0 && hipMemcpy(order, sim->d_order, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(MG_EDEVICE, "mg_work_order: copy failed");
    } else {
      for (int i = 0; i < n; i++) order[i] = i;  // no sort has run yet: the launches took the slots in order
    }
  }
  if (cost && n > 0 && hipMemcpy(cost, sim->d_cost, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(MG_EDEVICE, "mg_work_order: copy failed");
  *n_out = n;
  return MG_OK;
}

int mg_sim_kernel_layout(mg_sim* sim, int32_t* team_lanes, int32_t* compact) {
  if (!sim || !team_lanes || !compact) return fail(MG_EINVAL, "mg_sim_kernel_layout: bad arguments");
  *team_lanes = 0;
  *compact = 0;
  if (mgi::team_size(sim->host_model, sim->params.max_contacts) <= 0) return MG_OK;  // no instance fits: no team kernel
  return mgi::dispatch<mgi::InstanceOf>(sim->host_model, sim->params.max_contacts, sim->layout_n, team_lanes, compact);
}

int mg_model_team_lanes(const mg_model* model, int32_t max_contacts, int32_t* team_lanes) {
  if (!model || !team_lanes) return fail(MG_EINVAL, "mg_model_team_lanes: bad arguments");
  *team_lanes = mgi::team_size(*model, max_contacts);
  return MG_OK;
}

int mg_set_indexed(mg_sim* sim, int32_t which, const float* src, const int32_t* idx, int32_t n, void* stream) {
  if (!sim || !sim->bound || !src || (n > 0 && !idx)) return fail(MG_EINVAL, "mg_set_indexed: bad arguments");
  if (n == 0) return MG_OK;
  float* dst;
  int row;
  if (which == MG_SET_ROOT_STATE) {
    dst = sim->views.root_states;
    row = 13;
  } else if (which == MG_SET_DOF_STATE) {
    dst = sim->views.dof_state;
    row = 2 * sim->host_model.num_dofs;
  } else if (which == MG_SET_DOF_TARGET) {
    dst = const_cast<float*>(sim->views.dof_targets);
    row = sim->host_model.num_dofs;
    if (!dst) return fail(MG_EINVAL, "mg_set_indexed: no dof_targets bound");
  } else {
    return fail(MG_EINVAL, "mg_set_indexed: unknown target");
  }
  if (dst == src) return MG_OK;  // caller wrote into the bound buffer itself (gym views alias sim memory)
  const int total = n * row;
  // hand-task envs: actor ids are global (3 per env: hand, object, goal); DOF rows belong to the hand
  const int div = (which != MG_SET_ROOT_STATE && sim->host_model.obj_type) ? 3 : 1;
  hipLaunchKernelGGL(k_set_indexed, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, dst, src, idx, n,
                     row, div);
  return check_launch("mg_set_indexed");
}

int mg_compute_observations(const mg_task_params* tp, int32_t n, const float* root_states, const float* dof_state,
                            const float* dof_force, const float* sensors, const float* actions, float* potentials,
                            float* prev_potentials, float* up_vec, float* heading_vec, float* obs, void* stream) {
  if (!tp || n < 0 || !dof_state || !obs || !actions) return fail(MG_EINVAL, "mg_compute_observations: bad args");
  if (tp->task_id != MG_TASK_CARTPOLE && (!root_states || !potentials || !prev_potentials || !up_vec || !heading_vec))
    return fail(MG_EINVAL, "mg_compute_observations: locomotion task needs root/potential buffers");
  if (n == 0) return MG_OK;
  hipLaunchKernelGGL(k_observations, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, *tp, n, root_states,
                     dof_state, dof_force, sensors, actions, potentials, prev_potentials, up_vec, heading_vec, obs);
  return check_launch("mg_compute_observations");
}

int mg_compute_reward(const mg_task_params* tp, int32_t n, const float* obs, const float* actions,
                      const float* potentials, const float* prev_potentials, const int64_t* progress, int64_t* reset,
                      float* rew, void* stream) {
  if (!tp || n < 0 || !obs || !actions || !progress || !reset || !rew) return fail(MG_EINVAL, "mg_compute_reward");
  if (tp->task_id != MG_TASK_CARTPOLE && (!potentials || !prev_potentials))
    return fail(MG_EINVAL, "mg_compute_reward: locomotion task needs potentials");
  if (n == 0) return MG_OK;
  hipLaunchKernelGGL(k_reward, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, *tp, n, obs, actions,
                     potentials, prev_potentials, progress, reset, rew);
  return check_launch("mg_compute_reward");
}

static int hand_args_ok(const mg_task_params* tp, const mg_state_views& v, const mg_task_buffers* tb,
                        const char* who) {
  if (!v.dof_targets || !v.rigid_body_states || !v.sensors || !v.dof_force || !tb->prev_targets ||
      !tb->goal_states || !tb->reset_goal || !tb->successes || !tb->consecutive_successes ||
      !tb->reduce_scratch || !tb->actions_out)
    return fail(MG_EINVAL, std::string(who) + ": ShadowHand needs dof_targets, rigid_body_states, sensors, "
                                              "dof_force and the hand task buffers");
  if (tp->num_dofs <= 0 || tp->num_dofs > MG_MAX_HAND_DOFS || tp->num_actions > MG_MAX_HAND_DOFS)
    return fail(MG_EINVAL, std::string(who) + ": bad hand DOF / action count");
  // obs_map / state_map hold 256 columns; the fused kernel's LDS row holds 212 (checked at launch)
  if (tp->num_obs <= 0 || tp->num_obs > 256 || tp->num_states < 0 || tp->num_states > 256)
    return fail(MG_EINVAL, std::string(who) + ": bad hand observation / state count");
  return MG_OK;
}

int mg_pre_physics(mg_sim* sim, const mg_task_params* tp, const mg_state_views* views, const mg_task_buffers* tb,
                   int32_t n, void* stream) {
  if (!tp || !tb || !tb->actions) return fail(MG_EINVAL, "mg_pre_physics: bad args");
  mg_state_views v;
  int nd;
  if (sim) {
    if (!sim->bound) return fail(MG_EINVAL, "mg_pre_physics: sim not bound");
    v = sim->views;
    n = sim->n;
    nd = sim->host_model.num_dofs;
  } else {
    if (!views) return fail(MG_EINVAL, "mg_pre_physics: need views without a sim");
    v = *views;
    nd = tp->task_id == MG_TASK_SHADOW_HAND ? tp->num_dofs : (tp->task_id == MG_TASK_CARTPOLE ? 2 : tp->num_actions);
  }
  if (n == 0) return MG_OK;
  if (tp->task_id == MG_TASK_SHADOW_HAND) {
    int rc = hand_args_ok(tp, v, tb, "mg_pre_physics");
    if (rc) return rc;
    hipLaunchKernelGGL(k_hand_pre, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, *tp, v, *tb, n, nd);
  } else {
    if (!v.dof_actuation) return fail(MG_EINVAL, "mg_pre_physics: locomotion task needs dof_actuation");
    hipLaunchKernelGGL(k_pre_loco, dim3(grid_for(n * nd)), dim3(kBlock), 0, (hipStream_t)stream, *tp, v, *tb, n,
                       nd);
  }
  return check_launch("mg_pre_physics");
}

int mg_post_physics(mg_sim* sim, const mg_task_params* tp, const mg_state_views* views, const mg_task_buffers* tb,
                    int32_t n, void* stream) {
  if (!tp || !tb) return fail(MG_EINVAL, "mg_post_physics: bad args");
  if (tp->num_actions > 64) return fail(MG_EINVAL, "mg_post_physics: num_actions > 64");
  if (tp->num_agents > 1 && (64 % tp->num_agents != 0 || tp->num_agents > MG_MAX_AGENTS ||
                             (sim ? sim->n : n) % tp->num_agents != 0))
    return fail(MG_EINVAL, "mg_post_physics: num_agents must divide 64 and the actor count");
  mg_state_views v;
  if (sim) {
    if (!sim->bound) return fail(MG_EINVAL, "mg_post_physics: sim not bound");
    v = sim->views;
    n = sim->n;
  } else {
    if (!views) return fail(MG_EINVAL, "mg_post_physics: need views without a sim");
    v = *views;
  }
  if (n == 0) return MG_OK;
  if (tp->task_id == MG_TASK_SHADOW_HAND) {
    int rc = hand_args_ok(tp, v, tb, "mg_post_physics");
    if (rc) return rc;
    hipLaunchKernelGGL(k_hand_post, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, *tp, v, *tb, n,
                       tp->num_dofs);
    if (!tb->defer_finalize)
      hipLaunchKernelGGL(k_hand_finalize, dim3(1), dim3(64), 0, (hipStream_t)stream, *tp, *tb);
    return check_launch("mg_post_physics");
  }
  hipLaunchKernelGGL(k_post_physics, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, *tp, v, *tb, n);
  return check_launch("mg_post_physics");
}

// Work ordering, sort mode (kOrderSort): a counting sort of the env units by the last launch's row counts,
// descending (the largest first), in two grid-wide passes of 256-unit blocks.  Pass 1 (k_ohist): each block's
// histogram in LDS -- the lanes of one key aggregated into one LDS add per key and wave, since a few hot bins would
// otherwise serialise every add -- then one global atomic per block and used bin reserves the block's range inside
// the bin, and each unit keeps its rank inside its block's range.  Pass 2 (k_oscatter): the bins' starts (a block
// scan of the 256 totals) and each unit's slot.  Where a unit lands inside its bin never changes a result, only
// which units share a wave.  The step kernel that runs this permutation zeroes the totals for the next sort
// (MgOrder::tot_clear), so the launches carry no host-side state and a captured graph replays them any number of times.
// (Fusing the histogram into the step kernel -- a global add per env -- and placing by per-bin cursors measured far
// slower: one hot bin's atomics serialise, Ant 65,536 156.0 -> 108.5 M)
__global__ __launch_bounds__(256) void k_ohist(const unsigned char* __restrict__ cost, int nu,
                                               unsigned* __restrict__ tot, unsigned* __restrict__ bbase,
                                               unsigned short* __restrict__ rank) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int u = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const int key = u < nu ? 255 - (int)cost[u] : -1;
  unsigned r = 0u;
  unsigned long long rem = __ballot(key >= 0);
  while (rem) {
    const int leader = __builtin_ctzll(rem);
    const int k = __shfl(key, leader);
    const unsigned long long same = __ballot(key == k) & rem;
    unsigned base = 0u;
    if (lane == leader) base = atomicAdd(&h[k], (unsigned)__popcll(same));
    base = (unsigned)__shfl((int)base, leader);
    if ((same >> lane) & 1ull) r = base + (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    rem &= ~same;
  }
  __syncthreads();
  const unsigned c = h[threadIdx.x];
  bbase[(size_t)blockIdx.x * 256 + threadIdx.x] = c ? atomicAdd(&tot[256 * (blockIdx.x % kSortRep) + threadIdx.x], c) : 0u;
  if (u < nu) rank[u] = (unsigned short)r;
}
__global__ __launch_bounds__(256) void k_oscatter(const unsigned char* __restrict__ cost, int nu,
                                                  const unsigned* __restrict__ tot, const unsigned* __restrict__ bbase,
                                                  const unsigned short* __restrict__ rank, int* __restrict__ order) {
  __shared__ unsigned wsum[4], start[256];
  const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
  // the bin's total over the copies, and this block's copy's offset inside the bin (the copies before it)
  const int rep = (int)(blockIdx.x % kSortRep);
  unsigned v = 0u, roff = 0u;
#pragma unroll
  for (int k = 0; k < kSortRep; k++) {
    const unsigned x = tot[256 * k + threadIdx.x];
    roff += k < rep ? x : 0u;
    v += x;
  }
  unsigned inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned y = (unsigned)__shfl_up((int)inc, d);
    inc += lane >= d ? y : 0u;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  unsigned off = 0u;
  for (int w = 0; w < wv; w++) off += wsum[w];
  start[threadIdx.x] = off + inc - v + roff;
  __syncthreads();
  const int u = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (u < nu) {
    const int key = 255 - (int)cost[u];
    const unsigned pos = start[key] + bbase[(size_t)blockIdx.x * 256 + key] + rank[u];
    if (pos < (unsigned)nu) order[pos] = u;  // always, unless the totals were not cleared
  }
}

static int env_step(mg_sim* sim, const mg_task_params* tp, const mg_task_buffers* tb, const mg_replay* rp,
                    void* stream) {
  if (!sim || !sim->bound || !tp || !tb || !tb->actions || !tb->obs || !tb->rew || !tb->reset || !tb->progress ||
      !tb->timeout)
    return fail(MG_EINVAL, "mg_env_step: bad arguments");
  if (sim->has_hf)
    return fail(MG_EINVAL, rp ? "mg_env_step_replay: the fused step has no heightfield instance (mg_sim_set_heightfield is set)"
                              : "mg_env_step: the fused step has no heightfield instance (mg_sim_set_heightfield is set)");
  if (sim->link_forces)
    return fail(MG_EINVAL, rp ? "mg_env_step_replay: the fused step applies no link forces (mg_sim_set_link_forces is on)"
                              : "mg_env_step: the fused step applies no link forces (mg_sim_set_link_forces is on)");
  const bool hand = tp->task_id == MG_TASK_SHADOW_HAND;
  if (hand != (sim->host_model.obj_type != 0))
    return fail(MG_EINVAL, "mg_env_step: ShadowHand needs a model with a free object (and only it does)");
  if (hand) {
    int rc = hand_args_ok(tp, sim->views, tb, "mg_env_step");
    if (rc) return rc;
    if (tp->num_dofs != sim->host_model.num_dofs || tp->rb_per_env != sim->host_model.num_bodies + 2)
      return fail(MG_EINVAL, "mg_env_step: task DOF / rigid-body counts do not match the model");
  } else {
    if (tp->task_id != MG_TASK_CARTPOLE && (!tb->potentials || !tb->prev_potentials || !tb->up_vec || !tb->heading_vec))
      return fail(MG_EINVAL, "mg_env_step: locomotion task needs potential/up/heading buffers");
    if (tp->num_actions > sim->host_model.num_nodes && tp->task_id != MG_TASK_CARTPOLE)
      return fail(MG_EINVAL, "mg_env_step: more actions than DOFs");
    if (tp->num_actions > mgi::team_size(sim->host_model, sim->params.max_contacts))
      return fail(MG_EINVAL, "mg_env_step: more actions than lanes per actor");
  }
  if (tp->num_agents > 1) {
    // the agents of an env must be teams of one wave (ballot/shuffle exchange): A | 64/T
    const int T = mgi::team_size(sim->host_model, sim->params.max_contacts);
    if (T == 0 || tp->num_agents > MG_MAX_AGENTS || (64 / T) % tp->num_agents != 0 ||
        sim->n % tp->num_agents != 0)
      return fail(MG_EINVAL, "mg_env_step: num_agents must divide the envs per wave (64 / team size) "
                             "and the actor count");
  }
  if (tp->num_actions > 64 || tp->num_obs > 256 || tp->num_states > 256)
    return fail(MG_EINVAL, "mg_env_step: num_actions > 64, num_obs > 256 or num_states > 256");
  if (sim->order_mode == kOrderLists && !rp) {
    // the in-kernel lists alternate between two sets by the host's launch parity, which a captured graph would freeze
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return fail(MG_EINVAL, "mg_env_step: MIGYM_ORDER=lists cannot be captured into a graph (use sort or off)");
  }
  if (sim->order_mode != kOrderOff && !rp) {
    const int A = tp->num_agents > 1 ? tp->num_agents : 1;
    if (A != sim->order_agents) return fail(MG_EINVAL, "mg_env_step: num_agents differs from mg_sim_params.agents");
    // the last launch's row counts -> this one's order (every sort_every-th ordered launch from the second on)
    if (sim->order_mode == kOrderSort && sim->order_valid && (sim->order_steps - 1) % sim->sort_every == 0) {
      const int nu = sim->bq_cap, nb = (nu + 255) / 256;
      unsigned* bbase = sim->d_osort + kSortTot;
      unsigned short* rank = reinterpret_cast<unsigned short*>(sim->d_osort + kSortTot + 256 * (size_t)nb);
      unsigned* tot = sim->d_osort;
      hipLaunchKernelGGL(k_ohist, dim3(nb), dim3(256), 0, (hipStream_t)stream, sim->d_cost, nu, tot, bbase, rank);
      hipLaunchKernelGGL(k_oscatter, dim3(nb), dim3(256), 0, (hipStream_t)stream, sim->d_cost, nu, tot, bbase, rank,
                         sim->d_order);
    }
  }
  int rc = mgi::dispatch<mgi::RunEnvStep>(sim->host_model, sim->params.max_contacts, sim->layout_n, (hipStream_t)stream,
                                          (const mg_sim*)sim, tp, tb, rp);
  if (rc) return rc;
  if (sim->order_mode != kOrderOff && !rp) {  // the launch wrote the next one's lists / row counts
    sim->order_steps++;
    sim->order_valid = true;
  }
  if (hand && !tb->defer_finalize)  // consecutive_successes running mean from the step's partial sums
    hipLaunchKernelGGL(k_hand_finalize, dim3(1), dim3(64), 0, (hipStream_t)stream, *tp, *tb);
  return check_launch(rp ? "mg_env_step_replay" : "mg_env_step");
}

int mg_env_step(mg_sim* sim, const mg_task_params* tp, const mg_task_buffers* tb, void* stream) {
  return env_step(sim, tp, tb, nullptr, stream);
}

// the manual-reset copy of the task buffers: reset_idx draws from a stream of the counter RNG that no step uses
static mg_task_buffers manual_reset_buffers(const mg_task_buffers* tb) {
  mg_task_buffers t = *tb;
  t.step_counter = tb->step_counter | (1ull << 62);
  return t;
}

int mg_reset_idx(mg_sim* sim, const mg_task_params* tp, const mg_task_buffers* tb, const int32_t* ids, int32_t n,
                 void* stream) {
  if (!sim || !sim->bound || !tp || !tb || n < 0 || (n > 0 && !ids) || !tb->reset || !tb->progress)
    return fail(MG_EINVAL, "mg_reset_idx: bad arguments");
  if (n == 0) return MG_OK;
  const bool hand = tp->task_id == MG_TASK_SHADOW_HAND;
  if (hand) {
    int rc = hand_args_ok(tp, sim->views, tb, "mg_reset_idx");
    if (rc) return rc;
  } else if (tp->task_id != MG_TASK_CARTPOLE && (!tb->potentials || !tb->prev_potentials)) {
    return fail(MG_EINVAL, "mg_reset_idx: locomotion task needs potential buffers");
  }
  if (tp->num_agents > MG_MAX_AGENTS) return fail(MG_EINVAL, "mg_reset_idx: num_agents > MG_MAX_AGENTS");
  const mg_task_buffers t = manual_reset_buffers(tb);
  hipLaunchKernelGGL(k_reset_idx, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, *tp, sim->views, t, ids,
                     n, sim->n);
  return check_launch("mg_reset_idx");
}

int mg_hand_finalize(const mg_task_params* tp, const mg_task_buffers* tb, void* stream) {
  if (!tp || !tb || !tb->reduce_scratch || !tb->consecutive_successes)
    return fail(MG_EINVAL, "mg_hand_finalize: needs reduce_scratch and consecutive_successes");
  hipLaunchKernelGGL(k_hand_finalize, dim3(1), dim3(64), 0, (hipStream_t)stream, *tp, *tb);
  return check_launch("mg_hand_finalize");
}

int mg_env_step_replay(mg_sim* sim, const mg_task_params* tp, const mg_task_buffers* tb, const mg_replay* rp,
                       void* stream) {
  if (!rp || !rp->dof_state) return fail(MG_EINVAL, "mg_env_step_replay: bad replay state");
  if (sim && sim->host_model.obj_type && (!rp->root_states || !rp->rigid_body_states))
    return fail(MG_EINVAL, "mg_env_step_replay: hand tasks need root and rigid-body states");
  return env_step(sim, tp, tb, rp, stream);
}

// ---- dynamics tensors and the fused operational-space controller (dynamics_tensors.hpp)
size_t mg_osc_args_sizeof(void) { return sizeof(mg_osc_args); }

// the shared argument check: a bound, fixed-base sim
static int dynamics_sim_ok(const mg_sim* sim, const char* who, bool need_bound) {
  if (!sim) return fail(MG_EINVAL, std::string(who) + ": bad arguments");
  if (!sim->host_model.fixed_base)
    return fail(MG_EINVAL, std::string(who) + ": dynamics tensors need a fixed-base model (the base columns of gym's "
                                              "floating-base tensors are not implemented)");
  // hand-task envs hold three root rows each (articulation, object, goal): the kernels index one row per actor
  if (sim->host_model.obj_type)
    return fail(MG_EINVAL, std::string(who) + ": models with a free object (hand tasks) are not supported");
  if (!sim->d_dyn) return fail(MG_EINVAL, std::string(who) + ": the model has no DOFs or a body outside its nodes");
  if (need_bound && !sim->bound) return fail(MG_EINVAL, std::string(who) + ": sim not bound");
  return MG_OK;
}

// the checks the entry points of the three-launch tasks share: every argument given and the sim bound ...
static int task_args_ok(const mg_sim* sim, const void* params, const void* views, const mg_task_buffers* tb,
                        const char* who) {
  if (!sim || !params || !views || !tb) return fail(MG_EINVAL, std::string(who) + ": bad arguments");
  if (!sim->bound) return fail(MG_EINVAL, std::string(who) + ": sim not bound");
  return MG_OK;
}
// ... the buffers the VecTask.step tail of a *_post launch writes ...
static bool step_tail_bound(const mg_task_buffers* tb) {
  return tb->obs && tb->rew && tb->reset && tb->progress && tb->timeout;
}
// ... and the state views a *_post launch reads: the injected ones, or the sim's bound ones
static const mg_state_views& state_views(const mg_sim* sim, const mg_state_views* state) {
  return state ? *state : sim->views;
}

int mg_dynamics_bind(mg_sim* sim, const mg_dynamics_views* views) {
  if (int rc = dynamics_sim_ok(sim, "mg_dynamics_bind", false)) return rc;
  if (!views) return fail(MG_EINVAL, "mg_dynamics_bind: bad arguments");
  sim->dyn = *views;
  return MG_OK;
}

int mg_dynamics_refresh(mg_sim* sim, void* stream) {
  if (int rc = dynamics_sim_ok(sim, "mg_dynamics_refresh", true)) return rc;
  if (!sim->dyn.jacobian && !sim->dyn.mass_matrix) return fail(MG_EINVAL, "mg_dynamics_refresh: no tensor bound");
  const int blocks = (sim->n + mgd::kTeams - 1) / mgd::kTeams;
  hipLaunchKernelGGL(mgd::k_dynamics_refresh, dim3(blocks), dim3(64), mgd::scratch_bytes(sim->host_model.num_nodes),
                     (hipStream_t)stream, (const mgd::DynModel*)sim->d_dyn, sim->n, (const float*)sim->views.root_states,
                     (const float*)sim->views.dof_state, sim->views.env_props, sim->views.env_props_stride,
                     sim->dyn.jacobian, sim->dyn.mass_matrix);
  return check_launch("mg_dynamics_refresh");
}

int mg_osc_torques(mg_sim* sim, const mg_osc_args* a, void* stream) {
  if (int rc = dynamics_sim_ok(sim, "mg_osc_torques", true)) return rc;
  const int nd = sim->host_model.num_nodes - 1;
  if (!a || !a->dpose || !a->eef_vel || !a->out) return fail(MG_EINVAL, "mg_osc_torques: bad arguments");
  if (a->arm_dofs < 1 || a->arm_dofs > mgd::kOscMax || a->arm_dofs > nd)
    return fail(MG_EINVAL, "mg_osc_torques: arm_dofs must be 1..7 and at most the model's DOFs");
  if (a->jac_body < 1 || a->jac_body >= sim->host_model.num_bodies)
    return fail(MG_EINVAL, "mg_osc_torques: jac_body must name a body other than the base link");
  if (a->out_cols < 1 || a->out_cols > a->arm_dofs || a->out_stride < a->out_cols || a->eef_vel_stride < 6)
    return fail(MG_EINVAL, "mg_osc_torques: out_cols must be 1..arm_dofs, out_stride >= out_cols, eef_vel_stride >= 6");
  if ((a->jac_in == nullptr) != (a->mm_in == nullptr))
    return fail(MG_EINVAL, "mg_osc_torques: jac_in and mm_in are given together or not at all");
  mgd::OscParams p;
  p.arm_dofs = a->arm_dofs;
  p.jac_body = a->jac_body;
  p.out_cols = a->out_cols;
  p.nd = nd;
  p.dpose = a->dpose;
  p.eef_vel = a->eef_vel;
  p.eef_vel_stride = a->eef_vel_stride;
  for (int k = 0; k < 6; k++) { p.kp[k] = a->kp[k]; p.kd[k] = a->kd[k]; }
  for (int k = 0; k < mgd::kOscMax; k++) {
    p.kp_null[k] = a->kp_null[k];
    p.kd_null[k] = a->kd_null[k];
    p.default_dof_pos[k] = a->default_dof_pos[k];
    p.effort_limit[k] = a->effort_limit[k];
  }
  p.out = a->out;
  p.out_stride = a->out_stride;
  p.jac_in = a->jac_in;
  p.mm_in = a->mm_in;
  const mgd::DynModel* dm = (const mgd::DynModel*)sim->d_dyn;
  const float* root = sim->views.root_states;
  const float* dof = sim->views.dof_state;
  if (a->jac_in)
    hipLaunchKernelGGL(mgd::k_osc<true>, dim3((sim->n + 63) / 64), dim3(64), 0, (hipStream_t)stream, dm, sim->n, p, root,
                       dof, sim->views.env_props, sim->views.env_props_stride);
  else
    hipLaunchKernelGGL(mgd::k_osc<false>, dim3((sim->n + mgd::kTeams - 1) / mgd::kTeams), dim3(64),
                       mgd::scratch_bytes(sim->host_model.num_nodes), (hipStream_t)stream, dm, sim->n, p, root, dof,
                       sim->views.env_props, sim->views.env_props_stride);
  return check_launch("mg_osc_torques");
}


// ---- FrankaReachMA: the task layer around mg_sim_simulate (reach_task.hpp)
size_t mg_reach_params_sizeof(void) { return sizeof(mg_reach_params); }
size_t mg_reach_views_sizeof(void) { return sizeof(mg_reach_views); }

// the shared argument check: a bound fixed-base sim whose model and actor count match the task constants
static int reach_args_ok(const mg_sim* sim, const mg_reach_params* rp, const mg_reach_views* v,
                         const mg_task_buffers* tb, const char* who) {
  if (int rc = dynamics_sim_ok(sim, who, true)) return rc;
  if (int rc = task_args_ok(sim, rp, v, tb, who)) return rc;
  const int A = rp->num_agents, T = rp->num_targets;
  if (A < 1 || A > MG_MAX_AGENTS || T < 1 || T > A)
    return fail(MG_EINVAL, std::string(who) + ": num_agents must be 1..8 and num_targets 1..num_agents");
  if (rp->num_obs != 10 + 3 * T + 3 * (A - 1))
    return fail(MG_EINVAL, std::string(who) + ": num_obs must be 10 + 3 num_targets + 3 (num_agents - 1)");
  if (sim->n % A != 0) return fail(MG_EINVAL, std::string(who) + ": the actor count is no multiple of num_agents");
  const mg_model& m = sim->host_model;
  if (rp->num_dofs != m.num_nodes - 1 || rp->num_dofs < 7 || rp->num_dofs > mgr::kReachDofs ||
      rp->num_bodies != m.num_bodies)
    return fail(MG_EINVAL, std::string(who) + ": num_dofs (7..9) / num_bodies do not match the sim's model");
  if (rp->jac_body < 1 || rp->jac_body >= m.num_bodies || rp->eef_body < 0 || rp->eef_body >= m.num_bodies ||
      rp->hand_body < 0 || rp->hand_body >= m.num_bodies)
    return fail(MG_EINVAL, std::string(who) + ": jac_body / eef_body / hand_body out of range");
  if (!v->cube_states || !v->init_cube_states || !v->dof_targets || !v->dof_actuation)
    return fail(MG_EINVAL, std::string(who) + ": needs cube_states, init_cube_states, dof_targets and dof_actuation");
  return MG_OK;
}

int mg_reach_pre(mg_sim* sim, const mg_reach_params* rp, const mg_reach_views* views, const mg_task_buffers* tb,
                 void* stream) {
  if (int rc = reach_args_ok(sim, rp, views, tb, "mg_reach_pre")) return rc;
  if (!tb->actions) return fail(MG_EINVAL, "mg_reach_pre: needs actions");
  if (!sim->views.rigid_body_states)
    return fail(MG_EINVAL, "mg_reach_pre: the sim needs rigid_body_states bound (eef_vel is read from it)");
  if (!(rp->action_scale != 0.0f)) return fail(MG_EINVAL, "mg_reach_pre: action_scale must not be 0");
  if (sim->n == 0) return MG_OK;
  mgd::OscParams p;
  p.arm_dofs = 7;
  p.jac_body = rp->jac_body;
  p.out_cols = 6;   // _arm_control[:, :6] (franka_reach_MA.py:817)
  p.nd = rp->num_dofs;
  p.dpose = nullptr;
  p.eef_vel = sim->views.rigid_body_states + (size_t)13 * rp->eef_body + 7;
  p.eef_vel_stride = (long long)13 * rp->num_bodies;
  for (int k = 0; k < 6; k++) { p.kp[k] = rp->kp[k]; p.kd[k] = rp->kd[k]; }
  for (int k = 0; k < mgd::kOscMax; k++) {
    p.kp_null[k] = rp->kp_null[k];
    p.kd_null[k] = rp->kd_null[k];
    p.default_dof_pos[k] = rp->osc_default_dof_pos[k];
    p.effort_limit[k] = rp->effort_limit[k];
  }
  p.out = views->dof_actuation;
  p.out_stride = rp->num_dofs;
  p.jac_in = nullptr;
  p.mm_in = nullptr;
  mgd::OscActions oa;
  oa.actions = tb->actions;
  oa.actions_out = tb->actions_out;
  oa.clip_actions = rp->clip_actions;
  oa.action_scale = rp->action_scale;
  for (int k = 0; k < 6; k++) oa.cmd_limit[k] = rp->cmd_limit[k];
  hipLaunchKernelGGL(mgr::k_reach_pre, dim3((sim->n + mgd::kTeams - 1) / mgd::kTeams), dim3(64),
                     mgd::scratch_bytes(sim->host_model.num_nodes), (hipStream_t)stream,
                     (const mgd::DynModel*)sim->d_dyn, sim->n, p, oa, (const float*)sim->views.root_states,
                     (const float*)sim->views.dof_state, sim->views.env_props, sim->views.env_props_stride);
  return check_launch("mg_reach_pre");
}

int mg_reach_post(mg_sim* sim, const mg_reach_params* rp, const mg_reach_views* views, const mg_task_buffers* tb,
                  const mg_state_views* state, void* stream) {
  if (int rc = reach_args_ok(sim, rp, views, tb, "mg_reach_post")) return rc;
  if (!tb->actions || !step_tail_bound(tb))
    return fail(MG_EINVAL, "mg_reach_post: needs actions, obs, rew, reset, progress and timeout");
  const mg_state_views& s = state_views(sim, state);
  if (!s.dof_state || !s.rigid_body_states || !s.net_contact_forces)
    return fail(MG_EINVAL, "mg_reach_post: needs dof_state, rigid_body_states and net_contact_forces");
  const int n_envs = sim->n / rp->num_agents;
  if (n_envs == 0) return MG_OK;
  mgr::ReachState st{s.dof_state, s.rigid_body_states, s.net_contact_forces};
  hipLaunchKernelGGL(mgr::k_reach_post, dim3((n_envs + mgr::kEnvs - 1) / mgr::kEnvs), dim3(64), 0,
                     (hipStream_t)stream, *rp, *views, *tb, st, n_envs);
  return check_launch("mg_reach_post");
}

int mg_reach_reset_idx(mg_sim* sim, const mg_reach_params* rp, const mg_reach_views* views,
                       const mg_task_buffers* tb, const int32_t* ids, int32_t n, void* stream) {
  if (int rc = reach_args_ok(sim, rp, views, tb, "mg_reach_reset_idx")) return rc;
  if (n < 0 || (n > 0 && !ids) || !tb->reset || !tb->progress)
    return fail(MG_EINVAL, "mg_reach_reset_idx: bad arguments");
  const int n_envs = sim->n / rp->num_agents;
  if (n == 0 || n_envs == 0) return MG_OK;
  const mg_task_buffers t = manual_reset_buffers(tb);
  hipLaunchKernelGGL(mgr::k_reach_reset_idx, dim3((n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, *rp,
                     *views, t, sim->views.dof_state, ids, n, n_envs);
  return check_launch("mg_reach_reset_idx");
}

// ---- Anymal: the task layer around mg_sim_simulate (anymal_task.hpp)
size_t mg_anymal_params_sizeof(void) { return sizeof(mg_anymal_params); }
size_t mg_anymal_views_sizeof(void) { return sizeof(mg_anymal_views); }

// the shared argument check: a bound free-base 12-DOF sim whose body count matches the task constants
static int anymal_args_ok(const mg_sim* sim, const mg_anymal_params* ap, const mg_anymal_views* v,
                          const mg_task_buffers* tb, const char* who) {
  if (int rc = task_args_ok(sim, ap, v, tb, who)) return rc;
  const mg_model& m = sim->host_model;
  if (m.fixed_base || m.obj_type || m.num_nodes - 1 != MG_ANYMAL_DOFS)
    return fail(MG_EINVAL, std::string(who) + ": needs a free-base model of 12 DOFs without a free object");
  if (ap->num_bodies != m.num_bodies) return fail(MG_EINVAL, std::string(who) + ": num_bodies does not match the sim's model");
  if (ap->base_body < 0 || ap->base_body >= m.num_bodies)
    return fail(MG_EINVAL, std::string(who) + ": base_body out of range");
  for (int k = 0; k < 4; k++)
    if (ap->knee_body[k] < 0 || ap->knee_body[k] >= m.num_bodies)
      return fail(MG_EINVAL, std::string(who) + ": knee_body out of range");
  if (!v->commands || !v->dof_targets) return fail(MG_EINVAL, std::string(who) + ": needs commands and dof_targets");
  return MG_OK;
}

int mg_anymal_pre(mg_sim* sim, const mg_anymal_params* ap, const mg_anymal_views* views, const mg_task_buffers* tb,
                  void* stream) {
  if (int rc = anymal_args_ok(sim, ap, views, tb, "mg_anymal_pre")) return rc;
  if (!tb->actions) return fail(MG_EINVAL, "mg_anymal_pre: needs actions");
  if (sim->views.dof_targets != views->dof_targets)
    return fail(MG_EINVAL, "mg_anymal_pre: views.dof_targets is not the buffer the sim has bound as dof_targets");
  if (sim->n == 0) return MG_OK;
  const long long total = (long long)sim->n * MG_ANYMAL_DOFS;
  hipLaunchKernelGGL(mga::k_anymal_pre, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *ap,
                     tb->actions, tb->actions_out, views->dof_targets, total);
  return check_launch("mg_anymal_pre");
}

int mg_anymal_post(mg_sim* sim, const mg_anymal_params* ap, const mg_anymal_views* views, const mg_task_buffers* tb,
                   const mg_state_views* state, void* stream) {
  if (int rc = anymal_args_ok(sim, ap, views, tb, "mg_anymal_post")) return rc;
  if (!tb->actions || !step_tail_bound(tb))
    return fail(MG_EINVAL, "mg_anymal_post: needs actions, obs, rew, reset, progress and timeout");
  const mg_state_views& s = state_views(sim, state);
  if (!s.root_states || !s.dof_state || !s.dof_force || !s.net_contact_forces)
    return fail(MG_EINVAL, "mg_anymal_post: needs root_states, dof_state, dof_force and net_contact_forces");
  if (sim->n == 0) return MG_OK;
  mga::AnymalState st{s.root_states, s.dof_state, s.dof_force, s.net_contact_forces};
  hipLaunchKernelGGL(mga::k_anymal_post, dim3((sim->n + mga::kEnvs - 1) / mga::kEnvs), dim3(64), 0,
                     (hipStream_t)stream, *ap, *views, *tb, st, sim->n);
  return check_launch("mg_anymal_post");
}

int mg_anymal_reset_idx(mg_sim* sim, const mg_anymal_params* ap, const mg_anymal_views* views,
                        const mg_task_buffers* tb, const int32_t* ids, int32_t n, void* stream) {
  if (int rc = anymal_args_ok(sim, ap, views, tb, "mg_anymal_reset_idx")) return rc;
  if (n < 0 || (n > 0 && !ids) || !tb->reset || !tb->progress || !sim->views.root_states || !sim->views.dof_state)
    return fail(MG_EINVAL, "mg_anymal_reset_idx: bad arguments");
  if (n == 0 || sim->n == 0) return MG_OK;
  const mg_task_buffers t = manual_reset_buffers(tb);
  mga::AnymalState st{sim->views.root_states, sim->views.dof_state, sim->views.dof_force,
                      sim->views.net_contact_forces};
  hipLaunchKernelGGL(mga::k_anymal_reset_idx, dim3((n + mga::kEnvs - 1) / mga::kEnvs), dim3(64), 0,
                     (hipStream_t)stream, *ap, *views, t, st, ids, n, sim->n);
  return check_launch("mg_anymal_reset_idx");
}

// ---- Quadcopter: the task layer around mg_sim_simulate with link forces (quadcopter_task.hpp)
size_t mg_quadcopter_params_sizeof(void) { return sizeof(mg_quadcopter_params); }
size_t mg_quadcopter_views_sizeof(void) { return sizeof(mg_quadcopter_views); }

// the shared argument check: a bound free-base sim of 8 DOFs and 9 bodies, the rotor rows inside the force tensor
static int quadcopter_args_ok(const mg_sim* sim, const mg_quadcopter_params* qp, const mg_quadcopter_views* v,
                              const mg_task_buffers* tb, const char* who) {
  if (int rc = task_args_ok(sim, qp, v, tb, who)) return rc;
  const mg_model& m = sim->host_model;
  if (m.fixed_base || m.obj_type || m.num_nodes - 1 != MG_QUAD_DOFS || m.num_bodies != MG_QUAD_BODIES)
    return fail(MG_EINVAL, std::string(who) + ": needs a free-base model of 8 DOFs and 9 bodies without a free object");
  for (int k = 0; k < 4; k++)
    if (qp->rotor_body[k] < 0 || qp->rotor_body[k] >= MG_QUAD_BODIES)
      return fail(MG_EINVAL, std::string(who) + ": rotor_body out of range");
  if (!v->thrusts || !v->dof_targets || !v->forces)
    return fail(MG_EINVAL, std::string(who) + ": needs thrusts, dof_targets and forces");
  if (!sim->views.root_states || !sim->views.dof_state)
    return fail(MG_EINVAL, std::string(who) + ": needs root_states and dof_state");
  return MG_OK;
}

int mg_quadcopter_pre(mg_sim* sim, const mg_quadcopter_params* qp, const mg_quadcopter_views* views,
                      const mg_task_buffers* tb, void* stream) {
  if (int rc = quadcopter_args_ok(sim, qp, views, tb, "mg_quadcopter_pre")) return rc;
  if (!tb->actions || !tb->reset || !tb->progress) return fail(MG_EINVAL, "mg_quadcopter_pre: needs actions, reset and progress");
  if (sim->views.dof_targets != views->dof_targets || sim->views.rb_forces != views->forces)
    return fail(MG_EINVAL, "mg_quadcopter_pre: views.dof_targets / forces are not the buffers the sim has bound as "
                           "dof_targets / rb_forces");
  if (sim->n == 0) return MG_OK;
  hipLaunchKernelGGL(mgq::k_quad_pre, dim3((sim->n + mgq::kEnvs - 1) / mgq::kEnvs), dim3(64), 0, (hipStream_t)stream,
                     *qp, *views, *tb, sim->views.root_states, sim->views.dof_state, sim->n);
  return check_launch("mg_quadcopter_pre");
}

int mg_quadcopter_post(mg_sim* sim, const mg_quadcopter_params* qp, const mg_quadcopter_views* views,
                       const mg_task_buffers* tb, const mg_state_views* state, void* stream) {
  if (int rc = quadcopter_args_ok(sim, qp, views, tb, "mg_quadcopter_post")) return rc;
  if (!step_tail_bound(tb))
    return fail(MG_EINVAL, "mg_quadcopter_post: needs obs, rew, reset, progress and timeout");
  const mg_state_views& s = state_views(sim, state);
  if (!s.root_states || !s.dof_state) return fail(MG_EINVAL, "mg_quadcopter_post: needs root_states and dof_state");
  if (sim->n == 0) return MG_OK;
  hipLaunchKernelGGL(mgq::k_quad_post, dim3((sim->n + mgq::kEnvs - 1) / mgq::kEnvs), dim3(64), 0, (hipStream_t)stream,
                     *qp, *tb, (const float*)s.root_states, (const float*)s.dof_state, sim->n);
  return check_launch("mg_quadcopter_post");
}

int mg_quadcopter_reset_idx(mg_sim* sim, const mg_quadcopter_params* qp, const mg_quadcopter_views* views,
                            const mg_task_buffers* tb, const int32_t* ids, int32_t n, void* stream) {
  if (int rc = quadcopter_args_ok(sim, qp, views, tb, "mg_quadcopter_reset_idx")) return rc;
  if (n < 0 || (n > 0 && !ids) || !tb->reset || !tb->progress)
    return fail(MG_EINVAL, "mg_quadcopter_reset_idx: bad arguments");
  if (n == 0 || sim->n == 0) return MG_OK;
  const mg_task_buffers t = manual_reset_buffers(tb);
  hipLaunchKernelGGL(mgq::k_quad_reset_idx, dim3((n + mgq::kEnvs - 1) / mgq::kEnvs), dim3(64), 0, (hipStream_t)stream,
                     *qp, t, sim->views.root_states, sim->views.dof_state, ids, n, sim->n);
  return check_launch("mg_quadcopter_reset_idx");
}

// ---- Rendering: the ray caster over the collision geometry (render.hpp)
size_t mg_render_args_sizeof(void) { return sizeof(mg_render_args); }

// primitives per env: the actors' geoms, the free object and the goal, the extra boxes, the ground
static long render_prims(const mg_sim* sim, int num_boxes) {
  const mg_model& m = sim->host_model;
  const int A = sim->params.agents > 1 ? sim->params.agents : 1;
  return (long)A * m.num_geoms + (m.obj_type ? 2 : 0) + num_boxes + 1;
}

size_t mg_render_scratch_floats(const mg_sim* sim, int32_t n_sel, int32_t num_boxes) {
  if (!sim || n_sel < 1 || num_boxes < 0) return 0;
  const long P = render_prims(sim, num_boxes);
  if (P > mgrd::kMaxPrims) return 0;
  return (size_t)n_sel * (size_t)P * mgrd::kRec;
}

int mg_render(mg_sim* sim, const mg_render_args* a, void* stream) {
  if (!sim || !a) return fail(MG_EINVAL, "mg_render: bad arguments");
  if (!sim->bound || !sim->views.root_states || !sim->views.dof_state)
    return fail(MG_EINVAL, "mg_render: the sim's state is not bound (mg_sim_bind)");
  if (a->width < 1 || a->height < 1 || a->width > 16384 || a->height > 16384)
    return fail(MG_EINVAL, "mg_render: width and height must be 1..16384");
  if (!(a->fov_y > 0.0f) || !(a->fov_y < 3.14159265f)) return fail(MG_EINVAL, "mg_render: fov_y must be in (0, pi) radians");
  if (!a->rgb && !a->depth && !a->ids) return fail(MG_EINVAL, "mg_render: all outputs are NULL");
  if (a->n_sel < 1) return fail(MG_EINVAL, "mg_render: n_sel must be at least 1");
  if (a->num_boxes < 0 || (a->num_boxes > 0 && !a->boxes))
    return fail(MG_EINVAL, "mg_render: num_boxes must be >= 0 and boxes given when it is > 0");
  const long P = render_prims(sim, a->num_boxes);
  if (P > mgrd::kMaxPrims) return fail(MG_ECAPACITY, "mg_render: more than 512 primitives per env");
  if (!a->scratch || ((uintptr_t)a->scratch & 15)) return fail(MG_EINVAL, "mg_render: scratch is NULL or not 16-byte aligned");
  const mg_model& m = sim->host_model;
  const int A = sim->params.agents > 1 ? sim->params.agents : 1;
  const int n_env = sim->n / A;
  if (m.obj_type && A != 1) return fail(MG_EINVAL, "mg_render: a model with a free object has one actor per env");
  if (!a->env_ids && a->n_sel > n_env) return fail(MG_EINVAL, "mg_render: n_sel exceeds the env count");
  if (m.num_geoms < 0 || m.num_geoms > MG_MAX_GEOMS || m.hull_num_planes < 0 || m.hull_num_planes > MG_MAX_HULL_PLANES)
    return fail(MG_EINVAL, "mg_render: model tables out of range");
  for (int g = 0; g < m.num_geoms; g++)
    if (m.geom_node[g] < 0 || m.geom_node[g] >= m.num_nodes)
      return fail(MG_EINVAL, "mg_render: a geom names a node outside the model");
  {  // the camera must have a direction and a horizon
    float f[3], n2 = 0.0f;
    for (int k = 0; k < 3; k++) {
      f[k] = a->target_offset[k] - a->eye_offset[k];
      n2 += f[k] * f[k];
    }
    if (!(n2 > 0.0f) || !(f[0] * f[0] + f[1] * f[1] > 1e-12f * n2))
      return fail(MG_EINVAL, "mg_render: eye and target coincide, or the view is along z");
  }
  const long long npix = (long long)a->width * a->height;
  const long long tiles = (npix + mgrd::kTile - 1) / mgrd::kTile;
  if (tiles * a->n_sel > 0x7fffffffLL || (long long)a->n_sel * A > 0x7fffffffLL - mgrd::kTeams)
    return fail(MG_EINVAL, "mg_render: n_sel x image size exceeds the launch grid");
  const int rows_per_env = m.obj_type ? 3 : A;
  mgrd::SetupArgs s;
  s.m = sim->d_model;
  s.root = sim->views.root_states;
  s.dof = sim->views.dof_state;
  s.env_ids = a->env_ids;
  s.boxes = a->boxes;
  s.scratch = a->scratch;
  s.n_sel = a->n_sel;
  s.n_env = n_env;
  s.A = A;
  s.K = a->num_boxes;
  s.P = (int)P;
  s.rows_per_env = rows_per_env;
  const long teams = (long)a->n_sel * A;
  hipLaunchKernelGGL(mgrd::k_render_setup, dim3((unsigned)((teams + mgrd::kTeams - 1) / mgrd::kTeams)), dim3(64),
                     sizeof(float) * 12 * mgrd::kTeams * (size_t)m.num_nodes, (hipStream_t)stream, s);
  if (int rc = check_launch("mg_render (setup)")) return rc;
  mgrd::TraceArgs t;
  t.scratch = a->scratch;
  t.m = sim->d_model;
  t.root = sim->views.root_states;
  t.env_ids = a->env_ids;
  t.rgb = a->rgb;
  t.depth = a->depth;
  t.ids = a->ids;
  t.W = a->width;
  t.H = a->height;
  t.P = (int)P;
  t.n_env = n_env;
  t.rows_per_env = rows_per_env;
  t.follow = a->follow;
  t.tiles = (int)tiles;
  t.tan_half = tanf(0.5f * a->fov_y);
  for (int k = 0; k < 3; k++) {
    t.eye[k] = a->eye_offset[k];
    t.tgt[k] = a->target_offset[k];
  }
  hipLaunchKernelGGL(mgrd::k_render_trace, dim3((unsigned)(tiles * a->n_sel)), dim3(mgrd::kTile),
                     sizeof(float) * mgrd::kRec * (size_t)P + 3 * mgrd::kTile, (hipStream_t)stream, t);
  return check_launch("mg_render (trace)");
}

// ---- HumanoidAMP: the task layer around mg_sim_simulate (amp_task.hpp)
size_t mg_amp_params_sizeof(void) { return sizeof(mg_amp_params); }
size_t mg_amp_views_sizeof(void) { return sizeof(mg_amp_views); }

// the constants every AMP entry point relies on for its indexing
static int amp_params_ok(const mg_amp_params* ap, const mg_amp_views* v, const char* who) {
  if (!ap || !v) return fail(MG_EINVAL, std::string(who) + ": bad arguments");
  if (ap->num_bodies != MG_AMP_BODIES) return fail(MG_EINVAL, std::string(who) + ": num_bodies must be 15");
  for (int k = 0; k < MG_AMP_KEY_BODIES; k++)
    if (ap->key_body[k] < 0 || ap->key_body[k] >= MG_AMP_BODIES)
      return fail(MG_EINVAL, std::string(who) + ": key_body out of range");
  if (ap->num_amp_obs_steps < 2 || ap->num_amp_obs_steps > MG_AMP_MAX_OBS_STEPS)
    return fail(MG_EINVAL, std::string(who) + ": num_amp_obs_steps must be 2 .. 16");
  if (ap->state_init < MG_AMP_INIT_DEFAULT || ap->state_init > MG_AMP_INIT_HYBRID)
    return fail(MG_EINVAL, std::string(who) + ": unknown state_init");
  return MG_OK;
}

static int amp_motions_ok(const mg_amp_views* v, const char* who) {
  if (!v->motion_frames || !v->motion_index || !v->motion_time || v->num_motions < 1 || v->num_frames < 2)
    return fail(MG_EINVAL, std::string(who) + ": needs a motion table (motion_frames, motion_index, motion_time)");
  return MG_OK;
}

// a bound free-base 28-DOF, 15-body sim
static int amp_args_ok(const mg_sim* sim, const mg_amp_params* ap, const mg_amp_views* v, const mg_task_buffers* tb,
                       const char* who) {
  if (int rc = task_args_ok(sim, ap, v, tb, who)) return rc;
  if (int rc = amp_params_ok(ap, v, who)) return rc;
  const mg_model& m = sim->host_model;
  if (m.fixed_base || m.obj_type || m.num_nodes - 1 != MG_AMP_DOFS || m.num_bodies != MG_AMP_BODIES)
    return fail(MG_EINVAL, std::string(who) + ": needs a free-base model of 28 DOFs and 15 bodies without a free object");
  return MG_OK;
}

int mg_amp_pre(mg_sim* sim, const mg_amp_params* ap, const mg_amp_views* views, const mg_task_buffers* tb,
               void* stream) {
  if (int rc = amp_args_ok(sim, ap, views, tb, "mg_amp_pre")) return rc;
  if (!tb->actions) return fail(MG_EINVAL, "mg_amp_pre: needs actions");
  float* out = ap->pd_control ? views->dof_targets : views->dof_actuation;
  const float* bound = ap->pd_control ? sim->views.dof_targets : sim->views.dof_actuation;
  if (!out || out != bound)
    return fail(MG_EINVAL, ap->pd_control
                               ? "mg_amp_pre: views.dof_targets is not the buffer the sim has bound as dof_targets"
                               : "mg_amp_pre: views.dof_actuation is not the buffer the sim has bound as dof_actuation");
  if (sim->n == 0) return MG_OK;
  const long long total = (long long)sim->n * MG_AMP_DOFS;
  hipLaunchKernelGGL(mgh::k_amp_pre, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *ap,
                     tb->actions, tb->actions_out, out, total);
  return check_launch("mg_amp_pre");
}

int mg_amp_post(mg_sim* sim, const mg_amp_params* ap, const mg_amp_views* views, const mg_task_buffers* tb,
                const mg_state_views* state, void* stream) {
  if (int rc = amp_args_ok(sim, ap, views, tb, "mg_amp_post")) return rc;
  if (!step_tail_bound(tb) || !views->amp_obs || !views->terminate)
    return fail(MG_EINVAL, "mg_amp_post: needs obs, rew, reset, progress, timeout, amp_obs and terminate");
  const mg_state_views& s = state_views(sim, state);
  if (!s.root_states || !s.dof_state || !s.rigid_body_states || !s.net_contact_forces)
    return fail(MG_EINVAL, "mg_amp_post: needs root_states, dof_state, rigid_body_states and net_contact_forces");
  if (sim->n == 0) return MG_OK;
  mgh::AmpState st{s.root_states, s.dof_state, s.rigid_body_states, s.net_contact_forces};
  hipLaunchKernelGGL(mgh::k_amp_post, dim3((sim->n + mgh::kEnvs - 1) / mgh::kEnvs), dim3(64), 0, (hipStream_t)stream,
                     *ap, *views, *tb, st, sim->n);
  return check_launch("mg_amp_post");
}

int mg_amp_reset_idx(mg_sim* sim, const mg_amp_params* ap, const mg_amp_views* views, const mg_task_buffers* tb,
                     const int32_t* ids, int32_t n, void* stream) {
  if (int rc = amp_args_ok(sim, ap, views, tb, "mg_amp_reset_idx")) return rc;
  if (n < 0 || (n > 0 && !ids) || !tb->obs || !tb->reset || !tb->progress || !views->amp_obs || !views->terminate ||
      !sim->views.root_states || !sim->views.dof_state || !sim->views.rigid_body_states)
    return fail(MG_EINVAL, "mg_amp_reset_idx: bad arguments");
  if (ap->state_init != MG_AMP_INIT_DEFAULT)
    if (int rc = amp_motions_ok(views, "mg_amp_reset_idx")) return rc;
  if (n == 0 || sim->n == 0) return MG_OK;
  const mg_task_buffers t = manual_reset_buffers(tb);
  mgh::AmpState st{sim->views.root_states, sim->views.dof_state, sim->views.rigid_body_states,
                   sim->views.net_contact_forces};
  hipLaunchKernelGGL(mgh::k_amp_reset_idx, dim3((n + mgh::kEnvs - 1) / mgh::kEnvs), dim3(64), 0, (hipStream_t)stream,
                     *ap, *views, t, st, ids, n, sim->n);
  return check_launch("mg_amp_reset_idx");
}

int mg_amp_obs_demo(const mg_amp_params* ap, const mg_amp_views* views, const float* noise, uint64_t seed,
                    uint64_t counter, float* out, int32_t num_samples, void* stream) {
  if (int rc = amp_params_ok(ap, views, "mg_amp_obs_demo")) return rc;
  if (int rc = amp_motions_ok(views, "mg_amp_obs_demo")) return rc;
  if (num_samples < 0 || (num_samples > 0 && !out)) return fail(MG_EINVAL, "mg_amp_obs_demo: bad arguments");
  if (num_samples == 0) return MG_OK;
  hipLaunchKernelGGL(mgh::k_amp_obs_demo, dim3((num_samples + mgh::kEnvs - 1) / mgh::kEnvs), dim3(64), 0,
                     (hipStream_t)stream, *ap, *views, noise, seed, counter | (1ull << 61), out, num_samples);
  return check_launch("mg_amp_obs_demo");
}

}  // extern "C"
