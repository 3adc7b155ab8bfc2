// dynamics_tensors.hpp — Jacobian / mass-matrix tensors and the fused operational-space controller of fixed-base
// articulations (include/migym.h: mg_dynamics_refresh, mg_osc_torques).
//
// Layout: the step kernels' team design.  One 16-lane team per actor, four actors per 64-lane block (one wave), the
// model staged once per block in LDS, each team's link frames and inertias in its own LDS slice.  A lane owns the
// nodes tl, tl + 16, tl + 32: it walks its node's ancestor chain from the root (as fk() in team_physics.hpp: the
// deeper lanes repeat a few dozen FMAs instead of waiting a barrier per tree level).  Conventions are fk()'s and the
// oracle's forward_kinematics: node 0 is the fixed root, DOF j is node j + 1, spatial vectors are world-aligned at
// the root origin, [angular; linear].
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "device_math.hpp"

namespace mgd {
using namespace mg;

constexpr int kTeam = 16;                 // lanes per actor
constexpr int kTeams = 64 / kTeam;        // actors per block
constexpr int kOscMax = 7;                // controlled DOFs at most (mg_osc_args.arm_dofs)

// the model as the dynamics kernels read it (built by the host at mg_sim_create, one copy on the device)
struct DynModel {
  int32_t num_nodes, num_dofs, num_bodies, pad;
  unsigned long long anc[MG_MAX_NODES];   // bit k: node k is node i itself or one of its ancestors
  int32_t parent[MG_MAX_NODES];
  int32_t jtype[MG_MAX_NODES];
  int32_t body_node[MG_MAX_BODIES];
  // per node: rest rotation parent -> node (9, row-major), anchor t (3), axis (3), COM (3), inertia about the COM
  // (xx yy zz xy xz yz), mass, armature
  float nf[MG_MAX_NODES][26];
  float body_pos[MG_MAX_BODIES][3];       // body origin in its node's frame
};
static_assert(sizeof(DynModel) % 4 == 0, "DynModel is staged word by word");

inline void build_dyn_model(const mg_model& m, DynModel* d) {
  memset(d, 0, sizeof(*d));
  d->num_nodes = m.num_nodes;
  d->num_dofs = m.num_nodes - 1;
  d->num_bodies = m.num_bodies;
  for (int i = 0; i < m.num_nodes; i++) {
    d->parent[i] = i == 0 ? -1 : m.parent[i];
    d->anc[i] = (i == 0 ? 0ull : d->anc[m.parent[i]]) | (1ull << i);
    d->jtype[i] = m.jtype[i];
    const M3 R0 = quat_to_mat(m.r0[i][0], m.r0[i][1], m.r0[i][2], m.r0[i][3]);
    float* nf = d->nf[i];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) nf[3 * a + b] = R0.m[a][b];
    for (int a = 0; a < 3; a++) {
      nf[9 + a] = m.t[i][a];
      nf[12 + a] = m.axis[i][a];
      nf[15 + a] = m.com[i][a];
    }
    for (int a = 0; a < 6; a++) nf[18 + a] = m.inertia[i][a];
    nf[24] = m.mass[i];
    nf[25] = m.armature[i];
  }
  for (int b = 0; b < m.num_bodies; b++) {
    d->body_node[b] = m.body_node[b];
    for (int a = 0; a < 3; a++) d->body_pos[b][a] = m.body_pos[b][a];
  }
}

// one team's link frames, motion axes and inertias: rows per node in the block's dynamic LDS, sized by the model's
// own node count (the Franka's 10 nodes: 1.9 KB per team, 13 KB per block with the model, twelve blocks per CU; arrays
// of MG_MAX_NODES rows would hold a block at 36 KB and the CU at four)
struct TeamScratch {
  float (*R)[9];
  float (*x)[3];
  float (*S)[6];     // joint motion axis at the root origin [angular; linear]
  Sym6* Ic;          // link inertia at the root origin, then the composite of the node's subtree
  float (*F)[6];     // Ic S [moment; force]
  float* q;          // joint position of node i (q[0] unused)
  float (*dr)[2];    // this actor's [mass, armature] per node
};
constexpr int kNodeFloats = 9 + 3 + 6 + 21 + 6 + 1 + 2;
static_assert(sizeof(Sym6) == 21 * sizeof(float), "Sym6 is 21 packed floats");
inline size_t scratch_bytes(int num_nodes) { return sizeof(float) * kNodeFloats * kTeams * (size_t)num_nodes; }
__device__ __forceinline__ TeamScratch team_scratch(float* lds, int nn, int team) {
  float* b = lds + (size_t)kNodeFloats * nn * team;
  TeamScratch t;
  t.R = reinterpret_cast<float(*)[9]>(b);
  t.x = reinterpret_cast<float(*)[3]>(b + 9 * nn);
  t.S = reinterpret_cast<float(*)[6]>(b + 12 * nn);
  t.Ic = reinterpret_cast<Sym6*>(b + 18 * nn);
  t.F = reinterpret_cast<float(*)[6]>(b + 39 * nn);
  t.q = b + 45 * nn;
  t.dr = reinterpret_cast<float(*)[2]>(b + 46 * nn);
  return t;
}

__device__ __forceinline__ void stage_model(DynModel* dst, const DynModel* __restrict__ src) {
  const unsigned* s = reinterpret_cast<const unsigned*>(src);
  unsigned* d = reinterpret_cast<unsigned*>(dst);
  for (int k = threadIdx.x; k < (int)(sizeof(DynModel) / 4); k += blockDim.x) d[k] = s[k];
}

// Forward kinematics and CRBA composites of one actor by its team: fills ts->R, x, S, Ic (composite), for every node.
// `live` = the team has an actor (a dead team only keeps the block's barriers).  root: the actor's root row, dof: its
// (nD, 2) DOF rows, props: its env_props row or nullptr.
__device__ __forceinline__ void team_fk_crba(const DynModel* m, const TeamScratch* ts, int tl, bool live,
                                             const float* __restrict__ root, const float* __restrict__ dof,
                                             const float* __restrict__ props) {
  const int nn = m->num_nodes;
  if (live) {
    for (int i = tl; i < nn; i += kTeam) {
      ts->q[i] = i > 0 ? dof[2 * (i - 1)] : 0.0f;
      // domain randomization: the actor's own mass and armature (migym.h MG_EP_NODE rows), as the step kernels
      ts->dr[i][0] = props ? props[MG_EP_NODE_WIDTH * i] : m->nf[i][24];
      ts->dr[i][1] = props ? props[MG_EP_NODE_WIDTH * i + 1] : m->nf[i][25];
    }
  }
  __syncthreads();
  if (live) {
    float qx = root[3], qy = root[4], qz = root[5], qw = root[6];
    const float qn = 1.0f / sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
    qx *= qn; qy *= qn; qz *= qn; qw *= qn;
    const M3 Rr = quat_to_mat(qx, qy, qz, qw);
    const V3 x0 = ld3(root);
    for (int node = tl; node < nn; node += kTeam) {
      M3 R = Rr;
      V3 x = x0;
      SV S = szero();
      for (unsigned long long path = m->anc[node] & ~1ull; path; path &= path - 1) {
        const int k = __builtin_ctzll(path);
        const float* nf = m->nf[k];
        M3 R0;
        for (int a = 0; a < 3; a++)
          for (int b = 0; b < 3; b++) R0.m[a][b] = nf[3 * a + b];
        const M3 Rp0 = mul(R, R0);
        const V3 tp = mul(R, ld3(nf + 9));
        const V3 ax = ld3(nf + 12);
        const float qk = ts->q[k];
        if (m->jtype[k] == MG_JT_HINGE) {
          R = mul(Rp0, axis_angle(ax, qk));
          x = x + tp;
          const V3 sw = mul(R, ax);
          S = sv(sw, cross(x - x0, sw));
        } else {
          R = Rp0;
          const V3 sw = mul(Rp0, ax);
          x = x + tp + sw * qk;
          S = sv(v3(0, 0, 0), sw);
        }
      }
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) ts->R[node][3 * a + b] = R.m[a][b];
      ts->x[node][0] = x.x; ts->x[node][1] = x.y; ts->x[node][2] = x.z;
      ts->S[node][0] = S.a.x; ts->S[node][1] = S.a.y; ts->S[node][2] = S.a.z;
      ts->S[node][3] = S.l.x; ts->S[node][4] = S.l.y; ts->S[node][5] = S.l.z;
      // the link's spatial inertia at the root origin; under domain randomization the inertia scales with the mass
      const float* nf = m->nf[node];
      const float mass = ts->dr[node][0];
      const float isc = nf[24] > 0.0f ? mass / nf[24] : 1.0f;
      const V3 cc = x + mul(R, ld3(nf + 15)) - x0;
      const float* in = nf + 18;
      const float Il[3][3] = {{in[0] * isc, in[3] * isc, in[4] * isc}, {in[3] * isc, in[1] * isc, in[5] * isc},
                              {in[4] * isc, in[5] * isc, in[2] * isc}};
      float Tm[3][3], Iw[6];
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) Tm[a][b] = R.m[a][0] * Il[0][b] + R.m[a][1] * Il[1][b] + R.m[a][2] * Il[2][b];
      const int idx[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
      for (int k = 0; k < 6; k++) {
        const int a = idx[k][0], b = idx[k][1];
        Iw[k] = Tm[a][0] * R.m[b][0] + Tm[a][1] * R.m[b][1] + Tm[a][2] * R.m[b][2];
      }
      ts->Ic[node] = body_inertia(mass, cc, Iw);
    }
  }
  __syncthreads();
  // composites, leaves to root: element e of every node's inertia belongs to one lane, so the pass needs no
  // barrier between nodes (parent < child: a node is complete before it is added to its parent)
  if (live) {
    for (int e = tl; e < 21; e += kTeam)
      for (int i = nn - 1; i >= 1; i--) {
        float* pe = reinterpret_cast<float*>(&ts->Ic[m->parent[i]]) + e;
        *pe += reinterpret_cast<const float*>(&ts->Ic[i])[e];
      }
  }
  __syncthreads();
}

// F_i = Ic_i S_i for the nodes 1..last (one node per lane and round)
__device__ __forceinline__ void team_forces(const DynModel* m, const TeamScratch* ts, int tl, bool live, int last) {
  if (live) {
    for (int i = 1 + tl; i <= last; i += kTeam) {
      const float* s = ts->S[i];
      const SV f = mul(ts->Ic[i], sv(ld3(s), ld3(s + 3)));
      ts->F[i][0] = f.a.x; ts->F[i][1] = f.a.y; ts->F[i][2] = f.a.z;
      ts->F[i][3] = f.l.x; ts->F[i][4] = f.l.y; ts->F[i][5] = f.l.z;
    }
  }
  __syncthreads();
}

// M[r][c] (DOFs r, c): S_lo . (Ic_hi S_hi) when node lo is on node hi's chain (hi = the deeper of the two), + the
// armature on the diagonal.  (r, c) and (c, r) run the same operations on the same operands: M == M^T bit for bit.
__device__ __forceinline__ float mass_entry(const DynModel* m, const TeamScratch* ts, int r, int c) {
  const int hi = (r > c ? r : c) + 1, lo = (r > c ? c : r) + 1;
  float v = 0.0f;
  if ((m->anc[hi] >> lo) & 1ull) {
    const float* s = ts->S[lo];
    const float* f = ts->F[hi];
    v = s[0] * f[0] + s[1] * f[1] + s[2] * f[2] + s[3] * f[3] + s[4] * f[4] + s[5] * f[5];
  }
  if (r == c) v += ts->dr[hi][1];
  return v;
}

// Jacobian entry (body b's origin, row rw of [linear; angular], DOF d): [a x (o_b - p); a] for a hinge on b's
// chain, [a; 0] for a slide, zero off the chain
__device__ __forceinline__ float jac_entry(const DynModel* m, const TeamScratch* ts, int b, int rw, int d) {
  const int k = d + 1, nb = m->body_node[b];
  if (!((m->anc[nb] >> k) & 1ull)) return 0.0f;
  const float* s = ts->S[k];
  if (m->jtype[k] != MG_JT_HINGE) return rw < 3 ? s[3 + rw] : 0.0f;
  if (rw >= 3) return s[rw - 3];
  const float* R = ts->R[nb];
  const float* bp = m->body_pos[b];
  const V3 ob = v3(ts->x[nb][0] + R[0] * bp[0] + R[1] * bp[1] + R[2] * bp[2],
                   ts->x[nb][1] + R[3] * bp[0] + R[4] * bp[1] + R[5] * bp[2],
                   ts->x[nb][2] + R[6] * bp[0] + R[7] * bp[1] + R[8] * bp[2]);
  const V3 lin = cross(ld3(s), ob - ld3(ts->x[k]));
  return rw == 0 ? lin.x : (rw == 1 ? lin.y : lin.z);
}

// gym.refresh_jacobian_tensors + refresh_mass_matrix_tensors: each actor's blocks are contiguous and written by its
// team's lanes over consecutive addresses
__global__ __launch_bounds__(64) void k_dynamics_refresh(const DynModel* __restrict__ gm, int n,
                                                         const float* __restrict__ root_states,
                                                         const float* __restrict__ dof_state,
                                                         const float* __restrict__ env_props, int props_stride,
                                                         float* __restrict__ jac, float* __restrict__ mm) {
  __shared__ DynModel m;
  extern __shared__ float team_lds[];   // scratch_bytes(num_nodes)
  stage_model(&m, gm);
  __syncthreads();
  const int team = threadIdx.x / kTeam, tl = threadIdx.x % kTeam;
  const int actor = blockIdx.x * kTeams + team;
  const bool live = actor < n;
  const int ac = live ? actor : 0;
  const int nd = m.num_dofs, nb = m.num_bodies;
  const TeamScratch tsv = team_scratch(team_lds, m.num_nodes, team);
  const TeamScratch* ts = &tsv;
  team_fk_crba(&m, ts, tl, live, root_states + (size_t)13 * ac, dof_state + (size_t)2 * nd * ac,
               env_props ? env_props + (size_t)props_stride * ac : nullptr);
  team_forces(&m, ts, tl, live && mm != nullptr, nd);
  if (!live) return;
  if (mm) {
    float* o = mm + (size_t)nd * nd * actor;
    int r = 0, c = tl;
    for (int e = tl; e < nd * nd; e += kTeam) {
      while (c >= nd) { c -= nd; r++; }
      o[e] = mass_entry(&m, ts, r, c);
      c += kTeam;
    }
  }
  if (jac) {
    const int per_body = 6 * nd, tot = (nb - 1) * per_body;
    float* o = jac + (size_t)tot * actor;
    for (int e = tl; e < tot; e += kTeam) {
      const int b = e / per_body, rem = e - b * per_body, rw = rem / nd, d = rem - rw * nd;
      o[e] = jac_entry(&m, ts, b + 1, rw, d);
    }
  }
}

// ------------------------------------------------------------------------------------------------ OSC
struct OscParams {   // mg_osc_args by value, pointers included
  int32_t arm_dofs, jac_body, out_cols, nd;
  const float* dpose;
  const float* eef_vel;
  long long eef_vel_stride;
  float kp[6], kd[6], kp_null[kOscMax], kd_null[kOscMax], default_dof_pos[kOscMax], effort_limit[kOscMax];
  float* out;
  long long out_stride;
  const float* jac_in;
  const float* mm_in;
};

// torch's `%` on floats (the sign of the divisor), as the reference's wrap
__device__ __forceinline__ float floor_mod(float x, float y) {
  float r = fmodf(x, y);
  if (r != 0.0f && ((r < 0.0f) != (y < 0.0f))) r += y;
  return r;
}

// The controller's dense algebra for one actor, in registers, on M (7 x 7) and J (6 x 7) padded past arm_dofs with
// the identity / zeros (the padded DOFs then get zero torque and leave the others unchanged):
//   M = L L^T, Y = L^-1 J^T, A = Y^T Y = J M^-1 J^T = G G^T, u = J^T A^-1 (w - J un) + M un
// (the null-space term in its M^-1-free form, migym.h).  The solve runs in double on the fp32 M, J, w and un and rounds
// the torques to fp32: in fp32 it lost cond(A) eps32 of them (at cond(A) = 4.06e4 on the 17-node serial-arm tree, 0.16
// N m of 614, 6.2 x the worst error of fp32 LU inverses on the same inputs), in double its error is the inputs' and the
// output's rounding alone.  Returns false when a pivot of either factorisation fails the relative test
// s_j > kPivotTol X_jj (X = M or A; a NaN fails it, and so does every pivot of a diagonal entry <= 0, since
// s_j <= X_jj): the caller then writes zeros.  An absolute test s_j > 0 does not separate a singular matrix from a
// regular one: the exact pivot is 0 and the computed one has a random sign (with J of rank arm_dofs < 6, A = Y^T Y has
// rank arm_dofs; the fp32 Cholesky passed s > 0 on every pivot for 39 of 66 poses at arm_dofs = 5 on the MI355X, and
// an emulation in double does so for 31).
//
// kPivotTol, from two CPU measurements on the cases of tests/test_gpu_dynamics.py (tests/test_dynamics_host.py
// repeats both): (a) the largest first spurious pivot ratio |s_j| / A_jj of an FMA-free emulation of this function on
// the structurally singular cases (arm_dofs 3 and 5 on the serial-arm tree, 66 poses each) is 8.2e-7 in fp32, the
// precision of the inputs (3.3e-6 with a 4 x margin for the compiler's FMA contraction), and 1.4e-15 in double, the
// working precision; (b) the smallest true pivot ratio, in fp64, over every well-posed case the tests use is 5.97e-4
// (A on the arm_dofs = 6 tree; 1.02e-3 for A and 1.69e-2 for M on both Franka goldens, 0.38 for M on the tree).
// 4.4e-5 is the geometric mean of the fp32 figure and (b): 13 x above the one, 13 x below the other.  It is held
// against the fp32 figure because a pivot ratio is no better known than the fp32 inputs allow.
constexpr float kPivotTol = 4.4e-5f;
__device__ __forceinline__ bool osc_solve(const float (&M)[kOscMax][kOscMax], const float (&J)[6][kOscMax],
                                          const float (&w)[6], const float (&un)[kOscMax], float (&u)[kOscMax]) {
  using T = double;   // the solve's working precision (inputs and torques stay fp32)
  constexpr int N = kOscMax;
  bool ok = true;
  T L[N][N], di[N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    T s = M[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
    ok = ok && (s > T(kPivotTol) * M[j][j]);
    const T d = sqrt(fmax(s, T(1e-30)));
    di[j] = T(1) / d;
#pragma unroll
    for (int i = j + 1; i < N; i++) {
      T t = M[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) t -= L[i][k] * L[j][k];
      L[i][j] = t * di[j];
    }
  }
  T Y[N][6];
#pragma unroll
  for (int c = 0; c < 6; c++)
#pragma unroll
    for (int i = 0; i < N; i++) {
      T s = J[c][i];
#pragma unroll
      for (int k = 0; k < i; k++) s -= L[i][k] * Y[k][c];
      Y[i][c] = s * di[i];
    }
  T A[6][6];
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int b = 0; b <= a; b++) {
      T s = 0;
#pragma unroll
      for (int k = 0; k < N; k++) s += Y[k][a] * Y[k][b];
      A[a][b] = s;
    }
  T G[6][6], gi[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    T s = A[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) s -= G[j][k] * G[j][k];
    ok = ok && (s > T(kPivotTol) * A[j][j]);
    const T d = sqrt(fmax(s, T(1e-30)));
    gi[j] = T(1) / d;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      T t = A[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) t -= G[i][k] * G[j][k];
      G[i][j] = t * gi[j];
    }
  }
  T z[6];
#pragma unroll
  for (int a = 0; a < 6; a++) {   // g = w - J un, forward substitution in place
    T s = w[a];
#pragma unroll
    for (int k = 0; k < N; k++) s -= T(J[a][k]) * un[k];
#pragma unroll
    for (int k = 0; k < a; k++) s -= G[a][k] * z[k];
    z[a] = s * gi[a];
  }
#pragma unroll
  for (int a = 5; a >= 0; a--) {
    T s = z[a];
#pragma unroll
    for (int k = a + 1; k < 6; k++) s -= G[k][a] * z[k];
    z[a] = s * gi[a];
  }
#pragma unroll
  for (int i = 0; i < N; i++) {
    T s = 0;
#pragma unroll
    for (int k = 0; k < N; k++) s += T(M[i][k]) * un[k];
#pragma unroll
    for (int a = 0; a < 6; a++) s += J[a][i] * z[a];
    u[i] = (float)s;
  }
  return ok;
}

// where the team kernel takes an actor's dpose from when it is not p.dpose: the policy's action row
// (FrankaReachMA.pre_physics_step, franka_reach_MA.py:804-812; mg_reach_pre)
struct OscActions {
  const float* actions;   // (n, 6) raw actions
  float* actions_out;     // (n, 6) clamp(actions, +-clip_actions), or nullptr
  float clip_actions, action_scale;
  float cmd_limit[6];
};

// task-space command w and null-space torque un of one actor from its dpose row dp; DOFs past arm_dofs get zero
__device__ __forceinline__ void osc_inputs(const OscParams& p, const float* dp, int actor,
                                           const float* __restrict__ dof, float (&w)[6], float (&un)[kOscMax]) {
  const float* ev = p.eef_vel + (size_t)p.eef_vel_stride * actor;
#pragma unroll
  for (int a = 0; a < 6; a++) w[a] = p.kp[a] * dp[a] - p.kd[a] * ev[a];
  const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
#pragma unroll
  for (int i = 0; i < kOscMax; i++) {
    un[i] = 0.0f;
    if (i < p.arm_dofs) {
      const float q = dof[2 * i], qd = dof[2 * i + 1];
      un[i] = p.kd_null[i] * -qd + p.kp_null[i] * (floor_mod(p.default_dof_pos[i] - q + pi, two_pi) - pi);
    }
  }
}

// One team per actor: J's row and M's leading block are built in LDS from the state (the full tree's composites, so
// the gripper's inertia is in M) and never leave it.  ACT: dpose comes from the actor's action row (oa), clamped and
// scaled in the reference's operation order, and the clamped actions are written out; otherwise from p.dpose.  The
// body of k_osc<false> and of k_reach_pre (reach_task.hpp): one device code for both.
template <bool ACT>
__device__ __forceinline__ void osc_team(const DynModel* __restrict__ gm, int n, const OscParams& p,
                                         const float* __restrict__ root_states, const float* __restrict__ dof_state,
                                         const float* __restrict__ env_props, int props_stride,
                                         const OscActions* oa) {
  const int na = p.arm_dofs;
  float M[kOscMax][kOscMax], J[6][kOscMax], w[6], un[kOscMax], u[kOscMax];
  __shared__ DynModel m;
  extern __shared__ float team_lds[];   // scratch_bytes(num_nodes)
  __shared__ float MJ[kTeams][kOscMax * kOscMax + 6 * kOscMax];
  stage_model(&m, gm);
  __syncthreads();
  const int team = threadIdx.x / kTeam, tl = threadIdx.x % kTeam;
  const int actor = blockIdx.x * kTeams + team;
  const bool live = actor < n;
  const int ac = live ? actor : 0;
  const TeamScratch tsv = team_scratch(team_lds, m.num_nodes, team);
  const TeamScratch* ts = &tsv;
  const float* dof = dof_state + (size_t)2 * p.nd * ac;
  team_fk_crba(&m, ts, tl, live, root_states + (size_t)13 * ac, dof,
               env_props ? env_props + (size_t)props_stride * ac : nullptr);
  team_forces(&m, ts, tl, live, na);
  if (live) {
    float* mj = MJ[team];
    for (int e = tl; e < kOscMax * kOscMax; e += kTeam) {
      const int i = e / kOscMax, j = e - i * kOscMax;
      mj[e] = (i < na && j < na) ? mass_entry(&m, ts, i, j) : (i == j ? 1.0f : 0.0f);
    }
    for (int e = tl; e < 6 * kOscMax; e += kTeam) {
      const int a = e / kOscMax, j = e - a * kOscMax;
      mj[kOscMax * kOscMax + e] = j < na ? jac_entry(&m, ts, p.jac_body, a, j) : 0.0f;
    }
  }
  __syncthreads();
  if (!live) return;
  // every lane of the team runs the small dense solve on the same LDS values (broadcast reads): the lanes hold
  // identical u, and lane i writes torque i
  const float* mj = MJ[team];
#pragma unroll
  for (int i = 0; i < kOscMax; i++)
#pragma unroll
    for (int j = 0; j < kOscMax; j++) M[i][j] = mj[i * kOscMax + j];
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int j = 0; j < kOscMax; j++) J[a][j] = mj[kOscMax * kOscMax + a * kOscMax + j];
  if constexpr (ACT) {
    float dp[6];   // a product then a quotient: nothing here for FMA contraction to fuse
#pragma unroll
    for (int c = 0; c < 6; c++) {
      float a = oa->actions[(size_t)6 * actor + c];
      a = a < oa->clip_actions ? a : oa->clip_actions;
      a = a > -oa->clip_actions ? a : -oa->clip_actions;
      if (oa->actions_out && tl == c) oa->actions_out[(size_t)6 * actor + c] = a;
      dp[c] = (a * oa->cmd_limit[c]) / oa->action_scale;
    }
    osc_inputs(p, dp, actor, dof, w, un);
  } else {
    osc_inputs(p, p.dpose + (size_t)6 * actor, actor, dof, w, un);
  }
  const bool ok = osc_solve(M, J, w, un, u);
  float v = 0.0f, lim = 0.0f;
#pragma unroll
  for (int i = 0; i < kOscMax; i++)
    if (tl == i) { v = u[i]; lim = p.effort_limit[i]; }
  if (tl < p.out_cols) p.out[(size_t)p.out_stride * actor + tl] = ok ? fminf(fmaxf(v, -lim), lim) : 0.0f;
}

// INJECT: one lane per actor on the caller's J and M.  Otherwise one team per actor (osc_team).
template <bool INJECT>
__global__ __launch_bounds__(64) void k_osc(const DynModel* __restrict__ gm, int n, OscParams p,
                                            const float* __restrict__ root_states,
                                            const float* __restrict__ dof_state,
                                            const float* __restrict__ env_props, int props_stride) {
  if constexpr (INJECT) {
    const int na = p.arm_dofs;
    float M[kOscMax][kOscMax], J[6][kOscMax], w[6], un[kOscMax], u[kOscMax];
    const int actor = blockIdx.x * blockDim.x + threadIdx.x;
    if (actor >= n) return;
    const float* mi = p.mm_in + (size_t)na * na * actor;
    const float* ji = p.jac_in + (size_t)6 * na * actor;
#pragma unroll
    for (int i = 0; i < kOscMax; i++)
#pragma unroll
      for (int j = 0; j < kOscMax; j++) M[i][j] = (i < na && j < na) ? mi[i * na + j] : (i == j ? 1.0f : 0.0f);
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int j = 0; j < kOscMax; j++) J[a][j] = j < na ? ji[a * na + j] : 0.0f;
    osc_inputs(p, p.dpose + (size_t)6 * actor, actor, dof_state + (size_t)2 * p.nd * actor, w, un);
    const bool ok = osc_solve(M, J, w, un, u);
    float* o = p.out + (size_t)p.out_stride * actor;
#pragma unroll
    for (int i = 0; i < kOscMax; i++)
      if (i < p.out_cols) o[i] = ok ? fminf(fmaxf(u[i], -p.effort_limit[i]), p.effort_limit[i]) : 0.0f;
  } else {
    osc_team<false>(gm, n, p, root_states, dof_state, env_props, props_stride, nullptr);
  }
}

}  // namespace mgd
