/*
 * oracle.h — CPU restatement used ONLY as the parity checker and the CPU
 * baseline (tests/, __graft_entry__.smoke(), bench.py cpu_baseline leg).
 * Nothing in the product links or calls this library.
 *
 * PARITY STATUS
 *   obs / reward / reset bookkeeping: PINNED.  The restatement follows the
 *     reference's @torch.jit.script functions (tasks/ant.py:325-408,
 *     tasks/humanoid.py:323-413, tasks/cartpole.py:119-196,
 *     utils/torch_jit_utils.py:41-276) and VecTask.step ordering
 *     (tasks/base/vec_task.py:362-410); tests/test_oracle_golden.py checks it
 *     against tests/golden/jit_*.npz and trace_*.npz, produced by running the
 *     reference code itself (tests/golden/make_golden.py, make_traces.py).
 *   physics (gym.simulate): PARITY UNPINNED.  The reference physics is the
 *     closed isaacgym/PhysX binary (not in the reference tree, not installable
 *     offline).  This file restates the build's own documented algorithm
 *     (DESIGN.md §Physics): composite-rigid-body mass matrix + Cholesky in
 *     fp64 — deliberately NOT the O(n) articulated-body recursion the HIP
 *     kernels use — with the same contact set, PGS row order and integrator,
 *     and is pinned by analytic known-answer tests (free fall, energy,
 *     pendulum, joint limits, resting contact) in tests/test_oracle_physics.py.
 *   heightfield ground (orc_set_heightfield): the facet rule of DESIGN.md §15 in place of the plane z = 0 for
 *     every ground candidate, in fp64 (and in `real` in the fp32 twin); everything after the contact list -- the
 *     tangent basis, the Jacobian rows, the row order, PGS / TGS -- is the code the flat step runs.  Pinned on the
 *     CPU before it judges a kernel (tests/test_heightfield_oracle_host.py): bit-equal on a zero field, contact
 *     for contact against the definition in numpy, against its own flat step in a rotated frame on planes, and
 *     by analytic answers on one facet (rest, sliding, both tangent-basis branches) and in a V-shaped valley.
 */
#ifndef MIGYM_ORACLE_H
#define MIGYM_ORACLE_H
#include "../include/migym.h"

#ifdef __cplusplus
extern "C" {
#endif

/* counter-based uniform in [0,1): identical integer recipe on the GPU */
float orc_uniform(uint64_t seed, uint64_t env, uint64_t counter, uint32_t k);

/* gym.simulate on host buffers (gym layouts), fp64 internally, one actor per
 * row; `threads` OpenMP threads (0 = library default). */
int orc_simulate(const mg_model* m, const mg_sim_params* p, int32_t n, float* root_states, float* dof_state,
                 const float* dof_actuation, float* sensors, float* dof_force, int32_t threads);

/* The ground of every later call in this library: hf == NULL (the default) the plane z = 0; otherwise the heightfield
 * of DESIGN.md §15, read in every substep by orc_simulate, orc_simulate_views, orc_contacts, orc_contacts_full,
 * orc_contacts_marks, orc_contacts_phases and orc_step_flips.  hf->heights and hf->env_origins are HOST pointers,
 * kept and not copied; hf->hmax is used by orc_step_flips alone (the oracle culls nothing).  The env_origins row of an
 * actor is env_base + its index inside the call: env e of orc_simulate_views / orc_step_flips reads row env_base + e,
 * the one-actor hooks (orc_contacts*) read row env_base -- a caller that steps actor e through a one-row view passes
 * env_base = e.  The descriptor is process-wide and read-only during a call: set it between calls, never from inside
 * an OpenMP region.  Returns 0, or -1 on a NULL table, nx or ny < 2, dx <= 0 or a negative env_base (the plane then). */
int orc_set_heightfield(const mg_heightfield* hf, int32_t env_base);

/* gym.simulate on the full state views: object/goal root rows, PD targets and rigid-body states
 * of hand tasks included (views->dof_targets may be NULL = zero targets). */
int orc_simulate_views(const mg_model* m, const mg_sim_params* p, int32_t n, const mg_state_views* v,
                       int32_t threads);

/* Debug/KAT hooks for one actor: mass matrix (nv*nv row-major, includes the
 * armature + implicit damping/stiffness diagonal for substep h) and the
 * unconstrained generalized acceleration. */
int orc_mass_matrix(const mg_model* m, const mg_sim_params* p, const float* root13, const float* dof2,
                    double* M_out);
int orc_free_acceleration(const mg_model* m, const mg_sim_params* p, const float* root13, const float* dof2,
                          const float* tau, double* qacc_out);
/* contacts detected for one actor at the given state: returns count; writes
 * (node, px,py,pz, nx,ny,nz, depth, nodeB) records of 9 doubles */
int orc_contacts(const mg_model* m, const mg_sim_params* p, const float* root13, const float* dof2, double* out,
                 int32_t cap);
/* orc_contacts_full's records (nodeA, geomA, nodeB, geomB, p(3), n(3), d) with a 12th column of marks, thresholds moved out by delta (1 ambiguous pair, 2 ill-conditioned
 * normal, 4 within delta below its threshold, 8 at or above it); *pair_lost: an ambiguous decision left a
 * geom-object pair without a contact */
int orc_contacts_marks(const mg_model* m, const mg_sim_params* p, const float* root13, const float* dof2, double delta,
                       double* out, int32_t cap, int32_t* pair_lost);
/* per row of orc_contacts_marks (same arguments): the part of collide() that emitted it (1 geom on the ground, 2 the
 * object on the ground, 3 self pair, 4 / 5 / 6 hull vertices / faces / exact candidates, 7 another geom-object) */
int orc_contacts_phases(const mg_model* m, const mg_sim_params* p, const float* root13, const float* dof2, double delta,
                        int32_t* phases, int32_t cap);
/* egg narrowphase KAT hook (GJK + shrunk-core retry): kind 0 segment p0,p1 / kind 1 box c, R (row-major),
 * h, plus radius, vs the origin-centred ellipsoid e; out = point(3), normal(3), distance */
int orc_ellipsoid_contact(int32_t kind, const double* shape, double radius, const double* e, double* out);
/* edge-edge KAT hook: hand box c (3), R row-major (9), h (3) in the object box's frame (half extents hb);
 * out = point(3), normal(3), separation; returns 1 when generated */
int orc_box_box_edge(const double* shape, const double* hb, double off, double* out);
/* the convex-mesh geom's plane distance of n geom-frame points: out = (distance, face) per point */
int orc_hull_distance(const mg_model* m, const double* pl, int32_t n, double* out);
int orc_hull_core_contact(const mg_model* m, const double* shape, double rB, double off, double* out);
/* parity-test support: bit mask of the physics discontinuities env e's gym.simulate passes near (delta m / rad
 * of a contact / pair / limit threshold with the row in use; drives within df of saturation; seg_box_sat ties).
 * On a heightfield, from the fp64 run at every substep: 256 a ground candidate within 1e-5 cells of a cell edge or
 * diagonal with another plane behind it, 512 one whose geom the kernels' cull drops (c.z - (hmax - oz) - bound >= off)
 * -- both when the row is used or its gap within delta of the threshold, 256 also when only the other side touches --
 * and 1024 a candidate on another facet than at the substep before with its gap within delta of the threshold on
 * either of the two */
int orc_step_flips(const mg_model* m, const mg_sim_params* p, const mg_state_views* v, int32_t e, double delta,
                   double df);
/* test support: the contacts of env e's gym.simulate, substep by substep, without writing the views: records of 13
 * doubles (substep, nodeA, geomA, nodeB, p(3), n(3), d, the largest normal impulse the solve gave the row -- 0 for a
 * row it never used --, the tangential speed of the contact point at the substep's start); returns the count, or -1
 * on a model with a free object or with env_props bound */
int orc_step_rows(const mg_model* m, const mg_sim_params* p, const mg_state_views* v, int32_t e, double* out,
                  int32_t cap);
/* world poses of the gym rigid bodies (n_bodies x 13, velocity at body COM) */
int orc_rigid_body_states(const mg_model* m, const float* root13, const float* dof2, float* out);

int orc_compute_observations(const mg_task_params* tp, int32_t n, const float* root_states, const float* dof_state,
                             const float* dof_force, const float* sensors, const float* actions,
                             float* potentials, float* prev_potentials, float* up_vec, float* heading_vec,
                             float* obs);
int orc_compute_reward(const mg_task_params* tp, int32_t n, const float* obs, const float* actions,
                       const float* potentials, const float* prev_potentials, const int64_t* progress,
                       int64_t* reset, float* rew);
int orc_post_physics(const mg_task_params* tp, const mg_state_views* v, const mg_task_buffers* tb, int32_t n);
int orc_reset_idx(const mg_task_params* tp, const mg_state_views* v, const mg_task_buffers* tb, const int32_t* ids,
                  int32_t n_ids, int32_t n);
int orc_env_step(const mg_model* m, const mg_sim_params* p, const mg_task_params* tp, const mg_state_views* v,
                 const mg_task_buffers* tb, int32_t n, int32_t threads);

/* in-hand manipulation task layer (oracle_hand.c): ShadowHand full_state */
void orc_randomize_rotation(float r0, float r1, float* q);
int orc_hand_reward(const mg_task_params* tp, int32_t n, float max_episode_length, const float* object_pos,
                    const float* object_rot, const float* target_pos, const float* target_rot, const float* actions,
                    int64_t* reset, int64_t* reset_goal, int64_t* progress, float* successes, float* cons,
                    float* rew);
int orc_hand_pre_physics(const mg_model* m, const mg_task_params* tp, const mg_state_views* v,
                         const mg_task_buffers* tb, int32_t n);
int orc_hand_post_physics(const mg_model* m, const mg_task_params* tp, const mg_state_views* v,
                          const mg_task_buffers* tb, int32_t n);
int orc_hand_finalize(const mg_task_params* tp, const mg_task_buffers* tb);
int orc_hand_env_step(const mg_model* m, const mg_sim_params* p, const mg_task_params* tp,
                      const mg_state_views* v, const mg_task_buffers* tb, int32_t n, int32_t threads);

/* domain randomization (oracle_dr.c): restatements of mg_dr_apply / mg_dr_noise on host buffers */
int orc_dr_apply(const mg_dr_apply_args* a);
int orc_dr_noise(const mg_dr_noise_args* a);

#ifdef __cplusplus
}
#endif
#endif
