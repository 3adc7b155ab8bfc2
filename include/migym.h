/*
 * migym.h — C ABI of the MI355X-native physics-step + observation/reward path.
 *
 * This is the drop-in boundary that sits where the reference calls the closed
 * isaacgym tensor API.  Every entry point replaces one call
 * the reference's task layer makes on its hot path; the replaced call is cited
 * (paths relative to the reference checkout):
 *
 *   mg_sim_create        gym.create_sim + load_asset + create_env/create_actor loop
 *                        + prepare_sim              (tasks/base/vec_task.py:255-263,
 *                                                    tasks/ant.py:135-197)
 *   mg_sim_bind          gym.acquire_*_tensor + gymtorch.wrap_tensor
 *                                                   (tasks/ant.py:78-95, humanoid.py:75-95)
 *   mg_sim_simulate      gym.simulate(sim)          (tasks/base/vec_task.py:381-384)
 *   mg_sim_set_link_forces
 *                        gym.apply_rigid_body_force_tensors on articulation links
 *                                                   (tasks/quadcopter.py:330)
 *   mg_sim_set_heightfield
 *                        gym.add_triangle_mesh of a terrain_utils heightfield
 *                                                   (tasks/anymal_terrain.py:159-176), as facets of the grid
 *   mg_height_scan       AnymalTerrain.get_heights  (tasks/anymal_terrain.py:515-538)
 *   mg_set_indexed       gym.set_actor_root_state_tensor_indexed /
 *                        gym.set_dof_state_tensor_indexed
 *                                                   (tasks/ant.py:265-271, cartpole.py:153-155)
 *   mg_compute_observations   compute_{ant,humanoid}_observations / cartpole obs
 *                                                   (tasks/ant.py:374-408, humanoid.py:378-413,
 *                                                    cartpole.py:131-142)
 *   mg_compute_reward    compute_{ant,humanoid,cartpole}_reward
 *                                                   (tasks/ant.py:325-371, humanoid.py:323-375,
 *                                                    cartpole.py:180-196)
 *   (ShadowHand) mg_env_step also covers pre_physics_step's masked goal/env resets and
 *                        PD targets (shadow_hand.py:586-698) and compute_hand_reward's
 *                        global running mean (746-800, one finishing kernel).
 *   mg_env_step          one whole VecTask.step after the action tensor is on device:
 *                        clamp -> pre_physics_step -> simulate x controlFrequencyInv ->
 *                        post_physics_step (progress, masked reset_idx, obs, reward)
 *                        -> timeout_buf -> obs clamp  (tasks/base/vec_task.py:362-410,
 *                        tasks/ant.py:252-297) — no host synchronisation.
 *
 * Conventions
 *   - All tensors are device memory owned by the caller (PyTorch); pointers must
 *     stay valid for the call; layouts are the gym-visible ones:
 *       root_states (N*A, 13) f32 [px py pz qx qy qz qw vx vy vz wx wy wz]
 *       dof_state   (N*A*nD, 2) f32 [q, qdot];  sensors (N*A*S, 6) f32;
 *       dof_force   (N*A*nD) f32;  actions (N*A, nA) f32
 *       reset/progress/timeout buffers int64 (torch.long), as the reference.
 *   - Kernels are asynchronous on the caller's HIP stream (hipStream_t passed as
 *     void*; NULL = default stream).  No entry point synchronises the device.
 *   - Return 0 on success, a negative MG_E* code otherwise; mg_last_error()
 *     returns a thread-local message.  No C++ exception crosses the ABI.
 *   - One mg_sim per (process, device); calls on one handle are not thread-safe.
 */
#ifndef MIGYM_H
#define MIGYM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* stays 7 with the dynamics-tensor entry points (mg_dynamics_*, mg_osc_torques): they only add symbols, no existing
 * struct or call changes, and tests/test_abi.py pins mg_version() == 7 */
#define MG_VERSION 7

#define MG_MAX_NODES 40
#define MG_MAX_BODIES 40
#define MG_MAX_GEOMS 48
#define MG_MAX_PAIRS 192
#define MG_MAX_SENSORS 8
#define MG_MAX_TENDONS 8
#define MG_MAX_HAND_DOFS 32
#define MG_MAX_HULL_VERTS 160   /* the convex-mesh geom's hull (mg_model.hull_*) */
#define MG_MAX_HULL_PLANES 320

enum { MG_JT_FREE = 0, MG_JT_FIXED = 1, MG_JT_HINGE = 2, MG_JT_SLIDE = 3 };
enum { MG_GT_PLANE = 0, MG_GT_SPHERE = 1, MG_GT_CAPSULE = 2, MG_GT_BOX = 3, MG_GT_CYLINDER = 4, MG_GT_ELLIPSOID = 5,
       MG_GT_CONVEX = 6 /* convex mesh: the model's hull_* tables */ };
enum { MG_OK = 0, MG_EINVAL = -1, MG_EDEVICE = -2, MG_ENOMEM = -3, MG_ECAPACITY = -4 };
enum { MG_TASK_CARTPOLE = 0, MG_TASK_ANT = 1, MG_TASK_HUMANOID = 2, MG_TASK_SHADOW_HAND = 3 };
#define MG_MAX_AGENTS 8
enum { MG_SET_ROOT_STATE = 0, MG_SET_DOF_STATE = 1, MG_SET_DOF_TARGET = 2 };
/* coordinate space of applied rigid-body forces (gymapi.CoordinateSpace) */
enum { MG_ENV_SPACE = 0, MG_LOCAL_SPACE = 1, MG_GLOBAL_SPACE = 2 };
/* geom collision filter bits (mg_model.geom_filter) */
enum { MG_COLLIDE_GROUND = 1, MG_COLLIDE_OBJECT = 2 };

/* One articulation ("actor asset") as a dynamics tree of 1-DOF nodes.
 * Produced by migym/model.py (pack_model); field order == MODEL_DTYPE. */
typedef struct mg_model {
  int32_t num_nodes, num_dofs, fixed_base, num_bodies;
  int32_t num_geoms, num_pairs, num_sensors, nv;
  int32_t parent[MG_MAX_NODES];
  int32_t jtype[MG_MAX_NODES];
  int32_t limited[MG_MAX_NODES];
  int32_t node_body[MG_MAX_NODES];
  float t[MG_MAX_NODES][3];        /* joint anchor in parent node frame */
  float r0[MG_MAX_NODES][4];       /* rest rotation parent node -> node (xyzw) */
  float axis[MG_MAX_NODES][3];     /* joint axis, node frame (unit) */
  float mass[MG_MAX_NODES];
  float com[MG_MAX_NODES][3];      /* node frame */
  float inertia[MG_MAX_NODES][6];  /* about COM, node frame: xx yy zz xy xz yz */
  float armature[MG_MAX_NODES];
  float damping[MG_MAX_NODES];
  float stiffness[MG_MAX_NODES];
  float lower[MG_MAX_NODES];
  float upper[MG_MAX_NODES];
  int32_t body_node[MG_MAX_BODIES];
  int32_t body_parent[MG_MAX_BODIES];
  float body_pos[MG_MAX_BODIES][3];  /* body origin in its node frame */
  float body_quat[MG_MAX_BODIES][4];
  float body_com[MG_MAX_BODIES][3];  /* body COM in body frame */
  int32_t geom_type[MG_MAX_GEOMS];
  int32_t geom_node[MG_MAX_GEOMS];
  int32_t geom_body[MG_MAX_GEOMS];
  int32_t geom_filter[MG_MAX_GEOMS]; /* MG_COLLIDE_* bits */
  float geom_size[MG_MAX_GEOMS][3];
  float geom_pos[MG_MAX_GEOMS][3];   /* node frame */
  float geom_quat[MG_MAX_GEOMS][4];  /* node frame; capsule axis = local z */
  int32_t pair[MG_MAX_PAIRS][2];     /* self-collision geom pairs */
  int32_t sensor_body[MG_MAX_SENSORS];
  /* ---- position drives, fixed tendons and the free object of hand tasks
   * (shadow_hand.py:234-266, 684-698; shared.xml:55-72, 249-270) */
  float drive_kp[MG_MAX_NODES];      /* PD drive stiffness (MJCF <position kp>); > 0 = DOF_MODE_POS */
  float effort_limit[MG_MAX_NODES];  /* |drive force| limit (actuator forcerange) */
  int32_t num_tendons;
  int32_t gravity_off;               /* AssetOptions.disable_gravity of the articulation */
  int32_t tendon_dof[MG_MAX_TENDONS][2];
  float tendon_coef[MG_MAX_TENDONS][2];
  float tendon_range[MG_MAX_TENDONS][2];
  float tendon_limit_stiffness[MG_MAX_TENDONS];
  float tendon_damping[MG_MAX_TENDONS];
  /* One free rigid body per env next to the articulation (the manipulated object), plus a
   * kinematic goal actor.  Root-state rows per env are then [articulation, object, goal] and
   * rigid-body rows [articulation bodies..., object, goal]. */
  int32_t obj_type;                  /* 0 = none, MG_GT_BOX (block), MG_GT_ELLIPSOID (egg), MG_GT_CAPSULE (pen) */
  int32_t pair_mjcf;                 /* 1 = the pairs are explicit MJCF <pair>s (condim 1, margin 0): frictionless,
                                      * and in contact from zero distance (not the sim's contact offset) */
  float obj_mass;
  float obj_inertia[3];              /* principal moments, object frame (COM at the origin) */
  float obj_size[3];                 /* box half extents | ellipsoid semi-axes | capsule (radius, half length
                                      * along the object's z, 0) */
  float obj_lin_damping;
  float obj_ang_damping;
  float obj_gravity;                 /* 1 = the object falls under sim gravity */
  /* The convex-mesh collision geom (MG_GT_CONVEX; ShadowHand's robot0:C_forearm = mesh robot0:forearm_cvx,
   * robot.xml:8, shared_asset.xml:15), one per model: its hull in the geom frame (vertices, and outward
   * face planes n.x <= d inside).  geom_size of that geom = the hull's half extents about geom_pos. */
  int32_t hull_num_verts, hull_num_planes;
  float hull_vert[MG_MAX_HULL_VERTS][3];
  float hull_plane[MG_MAX_HULL_PLANES][4];
  /* Link velocity damping and cap of the articulation (gym AssetOptions.angular_damping /
   * max_angular_velocity; gym defaults 0.5 / 64: ant.py:152, humanoid.py:153-154, shadow_hand.py:240,
   * cartpole.py:86-87 keeps the defaults).  Damping acts on every link as the implicit couple
   * -c I_link w (a free link's w decays by 1/(1 + h c) per substep); the cap clamps every link's |w|
   * after the solve.  obj_max_ang_vel: the free object's cap (its damping is
   * obj_ang_damping).  A cap <= 0 disables it. */
  float link_ang_damping;
  float link_max_ang_vel;
  float obj_max_ang_vel;
  int32_t pad_model;
  /* Dry joint friction per DOF node: the MJCF joint `frictionloss` (the hand's default class, shared.xml:13:
   * 0.001), MuJoCo's constant friction torque bound, as the smooth law tau = -f tanh(qd / MG_FRICTIONLOSS_VS)
   * treated linearly implicitly like the damping (diagonal += h f / v_s sech^2); 0 = none */
  float frictionloss[MG_MAX_NODES];
} mg_model;
/* the regularization speed of the joint friction law (rad/s for hinges, m/s for slides) */
#define MG_FRICTIONLOSS_VS 0.01f

/* Simulation parameters (cfg['sim'] of the task YAML: Ant.yaml:42-61). */
typedef struct mg_sim_params {
  float dt;                 /* control dt (sim.dt) */
  int32_t substeps;         /* sim.substeps */
  float gravity[3];
  int32_t pos_iters;        /* physx.num_position_iterations: PGS sweeps per substep */
  float contact_offset;     /* physx.contact_offset: contacts generated below this gap */
  float rest_offset;        /* physx.rest_offset */
  float max_depen_vel;      /* physx.max_depenetration_velocity */
  float friction;           /* ground-plane friction coefficient */
  float baumgarte;          /* penetration recovery factor (build-defined) */
  float limit_margin;       /* joint-limit rows are built when within this distance */
  int32_t max_contacts;     /* per-actor contact capacity (<= MG_MAX_CONTACTS) */
  int32_t agents;           /* articulations per env (MA layouts; 1 otherwise) */
  int16_t solver_type;      /* MG_SOLVER_PGS (0, north_star) or MG_SOLVER_TGS (1, the reference's default,
                             * config.yaml:31): build-defined TGS, DESIGN.md §4 */
  int16_t vel_iters;        /* physx.num_velocity_iterations: TGS runs max(pos_iters, vel_iters) bias-free velocity
                             * sweeps after its sub-steps; unused by PGS.  (Two int16 keep the struct at 60 bytes:
                             * the kernels' argument layout, and so their code, stays as it was) */
} mg_sim_params;
#define MG_SOLVER_PGS 0
#define MG_SOLVER_TGS 1

/* Gym-visible state buffers the sim reads/writes (zero-copy, caller owned). */
typedef struct mg_state_views {
  float* root_states;       /* (N*A, 13) */
  float* dof_state;         /* (N*A*nD, 2) */
  const float* dof_actuation; /* (N*A*nD) effort, may be NULL (= zero) */
  float* sensors;           /* (N*A*S, 6), may be NULL */
  float* dof_force;         /* (N*A*nD), may be NULL */
  float* rigid_body_states; /* (N*A*nB, 13), may be NULL */
  const float* dof_targets; /* (N*A*nD) PD position targets (set_dof_position_target_tensor), may be NULL */
  /* gym.apply_rigid_body_force_tensors(sim, forces, None, space) (shadow_hand.py:700-708): forces
   * (N*A*nB, 3) in the rigid-body layout, applied at each body's centre of mass for every substep
   * of the next simulate.  Rows of the free object are applied.  Articulation rows are applied by
   * mg_sim_simulate once mg_sim_set_link_forces(sim, 1) is set (objectless models; below) and must be zero
   * otherwise: they are not read.  NULL = no forces.  The fused hand step writes this tensor (it owns the
   * random-force update). */
  float* rb_forces;
  int32_t rb_force_space;   /* MG_LOCAL_SPACE: body frame at the start of each substep; else world */
  int32_t env_props_stride; /* floats per row of env_props (mg_env_props_layout) */
  /* per-actor physical properties under domain randomization ((N*A, stride), see below); NULL = the
   * model's constants for every actor */
  const float* env_props;
  /* gym.acquire_net_contact_force_tensor / refresh_net_contact_force_tensor (franka_reach_MA.py:506, 563):
   * (N*A*nB, 3) in the rigid-body layout (hand tasks: the articulation's bodies, the object, the goal), the
   * world-frame net contact force on each body over the last substep (contact impulses / h; + on a contact's
   * side A, - on side B; the ground plane has no row).  Written by mg_sim_simulate and the fused step when bound;
   * NULL = not computed. */
  float* net_contact_forces;
} mg_state_views;

/* Task constants (cfg['env'] of the task YAML). */
typedef struct mg_task_params {
  int32_t task_id;          /* MG_TASK_* */
  int32_t num_obs;
  int32_t num_actions;
  int32_t max_episode_length;
  float dt;
  float clip_actions;       /* env.clipActions (inf if absent) */
  float clip_obs;           /* env.clipObservations (inf if absent) */
  float power_scale;        /* env.powerScale; Cartpole: maxEffort */
  float dof_vel_scale;
  float angular_velocity_scale;
  float contact_force_scale;
  float heading_weight;
  float up_weight;
  float actions_cost_scale;
  float energy_cost_scale;
  float joints_at_limit_cost_scale;
  float death_cost;
  float termination_height;
  float max_motor_effort;
  float reset_dist;         /* Cartpole resetDist */
  float target[3];          /* walk target (ant.py:105) */
  float start_pos[3];       /* actor start pose (ant.py:163-166) */
  float start_rot[4];
  float motor_effort[64];   /* per-DOF gear (actuator order, applied by DOF position) */
  float dof_lower[64];      /* task-side dof limits (swapped if lower>upper, ant.py:199-206) */
  float dof_upper[64];
  float initial_dof_pos[64];
  /* multi-agent layout (SURVEY.md §8(a) A-MA; franka_reach_MA.py:22-38, 598-612, 875-889):
   * actors are env-major (actor = env * num_agents + agent); an env resets only when all
   * of its agents are done (AND filter); obs rows append the other agents' torso positions
   * relative to self in cyclic-shift order.  num_agents = 1 for single-agent tasks. */
  int32_t num_agents;
  /* env.controlFrequencyInv: gym.simulate runs this many times per VecTask.step (vec_task.py:381-384)
   * while pre_physics_step / post_physics_step run once; 0 is taken as 1 */
  int32_t control_freq_inv;
  float agent_offset[8][3]; /* start-pose / target offset of each agent within its env */
  /* in-hand manipulation (MG_TASK_SHADOW_HAND; tasks/shadow_hand.py:40-118, ShadowHand.yaml) */
  int32_t num_fingertips;
  int32_t fingertip_body[8];          /* gym rigid-body index of each fingertip */
  int32_t actuated_dof[MG_MAX_HAND_DOFS]; /* action column -> DOF (actuator order) */
  int32_t max_consecutive_successes;
  int32_t use_relative_control;
  int32_t ignore_z_rot;               /* pen */
  int32_t obs_type;                   /* 0 full_state (211), 1 full (157), 2 full_no_vel (77), 3 openai (42) */
  int32_t rb_per_env;                 /* rigid-body rows per env (articulation bodies + object + goal) */
  int32_t num_dofs;                   /* hand DOFs (dof_state rows per env) */
  float dof_speed_scale;
  float act_moving_average;
  float dist_reward_scale;
  float rot_reward_scale;
  float rot_eps;
  float action_penalty_scale;
  float success_tolerance;
  float reach_goal_bonus;
  float fall_dist;
  float fall_penalty;
  float av_factor;
  float vel_obs_scale;
  float force_torque_obs_scale;
  float reset_position_noise;
  float reset_dof_pos_noise;
  float reset_dof_vel_noise;
  float object_start[3];             /* object_init_state position */
  float goal_displacement[3];        /* goal actor = goal_states + displacement */
  float goal_dz;                     /* goal_init = object_init + (0, 0, goal_dz) */
  /* asymmetric actor-critic (shadow_hand.py:125-131, 470-471): states_buf = the full_state layout */
  int32_t num_states;                /* 0 = no states buffer, else 211 */
  /* random object forces (shadow_hand.py:69-72, 196-199, 641-643, 700-708); force_scale 0 = off */
  int32_t object_rb;                 /* rigid-body row of the object within an env (object_rb_handles) */
  float force_scale;
  float force_decay_step;            /* forceDecay ** (dt / forceDecayInterval), fp32 (torch.pow) */
  float force_prob_lo;               /* forceProbRange */
  float force_prob_hi;
  float object_rb_mass;              /* object_rb_masses */
  /* observation column -> (segment << 8 | index) of the observationType layout (obs_map) and of the
   * full_state layout (state_map).  Filled by the library before a hand-task launch; callers need
   * not set them. */
  uint16_t obs_map[256];
  uint16_t state_map[256];
} mg_task_params;

/* Task-layer buffers (VecTask.allocate_buffers, vec_task.py:302-325). */
typedef struct mg_task_buffers {
  const float* actions;     /* (N*A, nA) raw policy actions (clamped inside) */
  float* actions_out;       /* (N*A, nA) clamped actions kept for obs (self.actions), may == NULL */
  float* obs;               /* (N*A, nO) obs_buf (unclamped, like the reference) */
  float* obs_clamped;       /* (N*A, nO) obs_dict['obs'] = clamp(obs_buf), may be NULL */
  float* rew;               /* (N*A) */
  int64_t* reset;           /* (N*A) */
  int64_t* progress;        /* (N*A) */
  uint8_t* timeout;         /* (N*A) torch.bool, like VecTask.timeout_buf after step */
  float* potentials;        /* (N*A) */
  float* prev_potentials;   /* (N*A) */
  float* up_vec;            /* (N*A, 3) */
  float* heading_vec;       /* (N*A, 3) */
  const float* noise;       /* (N*A, 2*nD) injected U(0,1) reset noise, or NULL = device RNG;
                             * ShadowHand: (N, 66) = [goal-only draw 4 | reset_idx draw 53 |
                             * reset_target_pose draw 4 | force-probability redraw 1 (U(0,1)) |
                             * force selection 1 (U(0,1)) | force direction 3 (N(0,1))]
                             * (shadow_hand.py:587, 610, 642-643, 704-706) */
  uint64_t seed;            /* device RNG seed (counter-based, keyed by global env id) */
  uint64_t step_counter;    /* VecTask.control_steps: RNG counter */
  int64_t env_offset;       /* global id of this shard's first env (multi-GPU); the RNG key of local actor a
                             * is the global actor id env_offset * num_agents + a, so a rollout does not
                             * depend on how the envs are sharded */
  /* in-hand manipulation (tasks/shadow_hand.py:186-219); unused by the other tasks */
  float* prev_targets;      /* (N, nD) */
  float* goal_states;       /* (N, 13) */
  int64_t* reset_goal;      /* (N) reset_goal_buf */
  float* successes;         /* (N) */
  float* consecutive_successes; /* (1) running mean (shadow_hand.py:795-798) */
  uint64_t* reduce_scratch; /* (2) device scratch: sum(resets), sum(successes * resets) */
  float* states;            /* (N, num_states) states_buf, may be NULL */
  float* random_force_prob; /* (N) per-env force probability, redrawn on reset; may be NULL */
  /* multi-GPU output path: when set, the step also writes each actor's row
   * [clamped obs (nO) | rew | reset] into this (N*A, nO + 2) f32 buffer, the message the obs gather
   * sends (migym/dist.py); the caller double-buffers it so the gather of step k overlaps step k+1 */
  float* out_pack;
  /* ShadowHand: 1 = leave this step's running-mean partial sums in reduce_scratch (the caller
   * all-reduces them over the ranks, then calls mg_hand_finalize); 0 = apply them in the step */
  int32_t defer_finalize;
  int32_t pad_tb;
} mg_task_buffers;

typedef struct mg_sim mg_sim;

/* ---- domain randomization (tasks/base/vec_task.py:612-842, utils/dr_utils.py) ----
 * The reference re-sets actor properties through the gym property setters in a per-env Python loop.
 * Here the per-actor physical properties live in one device table, env_props (N*A rows of `stride`
 * floats, bound through mg_state_views.env_props), which mg_dr_apply rewrites for the actors being
 * randomized and the physics kernels read instead of the model's constants.  Row layout (offsets
 * from mg_env_props_layout):
 *   MG_EP_NODE    num_nodes x MG_EP_NODE_WIDTH (9): [mass, armature, damping, stiffness, lower, upper, drive kp,
 *                 effort, frictionloss]
 *                 (mass of the node's body; its inertia scales with mass / model mass:
 *                 set_actor_rigid_body_properties(..., recomputeInertia=True))
 *   MG_EP_GEOM    num_geoms: friction of each collision shape (a contact's friction is the mean of
 *                 its two shapes'; the ground plane's is mg_sim_params.friction)
 *   MG_EP_TENDON  num_tendons x 2: [limit stiffness, damping]
 *   MG_EP_OBJECT  4: [mass, friction, scale, 0] of the free object (scale: half extents x s,
 *                 mass x s^3, inertia x s^5) */
enum { MG_EP_NODE = 0, MG_EP_GEOM = 1, MG_EP_TENDON = 2, MG_EP_OBJECT = 3 };
#define MG_EP_NODE_WIDTH 9
enum { MG_DR_UNIFORM = 0, MG_DR_GAUSSIAN = 1, MG_DR_LOGUNIFORM = 2 };
enum { MG_DR_ADDITIVE = 0, MG_DR_SCALING = 1 };
enum { MG_DR_SCHED_NONE = 0, MG_DR_SCHED_LINEAR = 1, MG_DR_SCHED_CONSTANT = 2 };

/* one randomized attribute (dr_utils.generate_random_samples / apply_random_samples) */
typedef struct mg_dr_desc {
  int32_t distribution;     /* MG_DR_UNIFORM / GAUSSIAN (range = [mu, std]) / LOGUNIFORM */
  int32_t operation;        /* MG_DR_ADDITIVE / MG_DR_SCALING */
  int32_t schedule;         /* MG_DR_SCHED_* */
  int32_t schedule_steps;
  int32_t num_buckets;      /* > 0: get_bucketed_val over the unscheduled range */
  int32_t after_setup;      /* 0: its property holds a setup_only attribute (randomized on the first call only) */
  float range[2];
} mg_dr_desc;
/* one element of an attribute: env_props column, descriptor, original value (og_prop) */
typedef struct mg_dr_attr {
  int32_t slot;
  int32_t desc;
  float og;
  int32_t pad;
} mg_dr_attr;

typedef struct mg_dr_apply_args {
  const mg_dr_desc* descs;  /* device */
  const mg_dr_attr* attrs;  /* device, nattr */
  int32_t nattr;
  int32_t stride;           /* env_props row length */
  int32_t n;                /* actors */
  int32_t frequency;        /* randomization_params.frequency */
  int32_t first;            /* first_randomization: every actor, setup_only attributes included */
  int32_t increment;        /* randomize_buf += 1 before the test (post_physics_step's increment) */
  int64_t last_step;        /* gym.get_frame_count (schedules) */
  float* env_props;         /* (n, stride) */
  const int64_t* reset_mask;/* (n) reset_buf of the resetting step (ignored with first) */
  int64_t* randomize_buf;   /* (n) */
  const float* samples;     /* (n, nattr) injected samples (generate_random_samples output), or NULL */
  uint64_t seed;            /* device RNG: counter-based, keyed by (global actor id, counter, attr) */
  uint64_t counter;
  int64_t env_offset;
} mg_dr_apply_args;

/* noise_lambda of randomization_params.observations / .actions (vec_task.py:684-720), in the
 * reference's fp32 operation order:
 *   x = op(x, ((corr * c_scale + c_shift) + z * scale) + shift)
 * gaussian: z ~ N(0,1), scale = var, shift = mu, c_scale = var_corr, c_shift = mu_corr;
 * uniform:  z ~ U(0,1), scale = hi - lo, shift = lo, c_scale = hi_corr - lo_corr, c_shift = lo_corr
 * (corr is N(0,1) in both, as the reference draws it with randn_like).  Optional clamp into x_clamped. */
typedef struct mg_dr_noise_args {
  float* x;                 /* (n) in/out */
  float* x_clamped;         /* (n) clamp(x, +-clip) or NULL */
  float clip;
  int32_t distribution;     /* MG_DR_GAUSSIAN or MG_DR_UNIFORM */
  int32_t operation;        /* MG_DR_ADDITIVE / MG_DR_SCALING */
  int32_t refresh_corr;     /* draw a new corr tensor first ("corr" absent from dr_randomizations) */
  float* corr;              /* (n) persistent correlated noise */
  int64_t n;
  float scale, shift;       /* schedule applied by the caller */
  float c_scale, c_shift;
  const float* injected;    /* (n) per-call draws (randn_like / rand_like), or NULL = device RNG */
  const float* injected_corr; /* (n) corr draws when refreshing, or NULL */
  uint64_t seed;
  uint64_t counter;
  int64_t elem_offset;      /* global index of element 0 (multi-GPU shards) */
  uint32_t key;             /* RNG stream of this tensor */
  int32_t pad;
} mg_dr_noise_args;

int mg_env_props_layout(const mg_model* m, int32_t offsets[4]);   /* returns the row stride (floats) */
int mg_env_props_defaults(const mg_model* m, float* row);           /* host: one row of model values */
int mg_dr_apply(const mg_dr_apply_args* a, void* stream);
int mg_dr_noise(const mg_dr_noise_args* a, void* stream);
/* replace the simulation parameters (gym.set_sim_params; DR of sim_params.gravity) */
int mg_sim_set_params(mg_sim* sim, const mg_sim_params* params);

const char* mg_last_error(void);
int mg_version(void);
size_t mg_model_sizeof(void);
size_t mg_task_params_sizeof(void);
size_t mg_task_buffers_sizeof(void);
size_t mg_sim_params_sizeof(void);
size_t mg_state_views_sizeof(void);
size_t mg_dr_desc_sizeof(void);
size_t mg_dr_apply_args_sizeof(void);
size_t mg_dr_noise_args_sizeof(void);
/* profiling aid (phase-timing build only, see isaacgymenvs-ma_amd/build.py --timing): MG_NUM_PHASES counters */
#define MG_NUM_PHASES 32
int mg_debug_phase_cycles(uint64_t* out, int32_t reset);
/* ... and the per-item rows behind it (an item = one wave's teams; cap items of MG_NUM_PHASES counts each) */
int mg_debug_phase_waves(uint64_t* out, int32_t cap);
/* test aid: the contact list of the first substep mg_sim_simulate would run from the bound state views, built by the
 * step kernel's own collide path (the instance and layout the dispatcher picks for mg_sim_simulate; non-DR, PGS).
 * count[a] = actor a's contacts; out[(a * cap + c) * 11 ..] = (nodeA, geomA, nodeB, geomB, point[3], normal[3],
 * gap) of its contact c, ids -1 = ground, -2 = the free object.  out: num_actors * cap * 11 floats, count:
 * num_actors ints (device memory).  cap below min(max_contacts, the instance's capacity) is MG_EINVAL.  Writes no
 * state. */
int mg_debug_contacts(mg_sim* sim, float* out, int32_t* count, int32_t cap, void* stream);

int mg_sim_create(const mg_model* model, const mg_sim_params* params, int32_t num_envs, int32_t device,
                  mg_sim** out);
int mg_sim_bind(mg_sim* sim, const mg_state_views* views);
int mg_sim_simulate(mg_sim* sim, void* stream);
/* Link forces (gym.apply_rigid_body_force_tensors on articulation links; torques are not built).  enable != 0: every
 * mg_sim_simulate reads each articulation row of the bound views.rb_forces ((N*A*nB, 3), nB = model.num_bodies) and
 * applies it at that body's centre of mass in every substep, in views.rb_force_space (MG_LOCAL_SPACE: the body's
 * frame of each substep's own start; else the env frame).  The tensor is read at every simulate and never cleared.
 * The launch then takes instances of its own, in the classic team layout at every batch size, and
 * mg_sim_simulate fails (nothing launched or written) with a NULL rb_forces, a model with a free object, env_props
 * bound, the compact layout pinned, or more bodies than the instance has nodes; mg_env_step and mg_env_step_replay
 * fail while it is on.  enable == 0 (the default): exactly the behaviour without this call. */
int mg_sim_set_link_forces(mg_sim* sim, int32_t enable);
/* Heightfield terrain (the ground of the reference's terrain tasks, tasks/anymal_terrain.py): fp32
 * heights in metres on a grid of square cells, heights[i * ny + j] at world (x0 + i dx, y0 + j dx) -- the index order of
 * the reference's height_samples[px, py].  env_origins: NULL, or (N, 3) fp32, actor a's local point (x, y, z) sitting
 * at world (x + ox, y + oy, z + oz).  hmax: an upper bound of heights, supplied by the caller (the ground-contact cull
 * relies on it).  heights and env_origins are device pointers, kept and not copied: the caller keeps them alive and may
 * rewrite their contents between launches. */
typedef struct mg_heightfield {
  const float* heights;
  int32_t nx, ny;           /* >= 2 each */
  float dx, x0, y0, hmax;
  const float* env_origins;
} mg_heightfield;
size_t mg_heightfield_sizeof(void);
/* hf != NULL: every later mg_sim_simulate and mg_debug_contacts takes each ground candidate against the triangular
 * facet of the field under it instead of the plane z = 0: the point is clamped to the grid rectangle, the cell's
 * facets are split by the diagonal from (i, j) to (i + 1, j + 1), the contact has the facet's normal n, the gap
 * (z - h) n.z - r and the point e - r n (DESIGN.md §15 has the formulas and the limits: a candidate sees only the facet
 * directly under it).  The launch then takes instances of its own, in the classic team layout at every batch size, and
 * fails (nothing launched or written) on a model with a free object, with env_props bound, with the compact layout
 * pinned, or with link forces on; mg_env_step and mg_env_step_replay fail while a field is set.  Fails on a NULL
 * table, nx or ny < 2, or a dx that is not finite and positive.  hf == NULL (the default): the plane, exactly the
 * behaviour without this call. */
int mg_sim_set_heightfield(mg_sim* sim, const mg_heightfield* hf);
/* The terrain height under a pattern of points that turns with each actor's yaw (get_heights, tasks/anymal_terrain.py:
 * 515-538): points (P, 2) fp32 on the device, out (N, P).  Per actor and point: the point is rotated by the yaw of the
 * bound root quaternion (quat_apply_yaw: x and y zeroed, normalised), the root's x, y and the env origin are added,
 * px = trunc((X - x0) / dx) clipped to [0, nx - 2], py likewise, out = min(H[px][py], H[px + 1][py + 1]) - oz.
 * Asynchronous on `stream`.  Fails without a field set. */
int mg_height_scan(mg_sim* sim, const float* points, int32_t num_points, float* out, void* stream);
int mg_sim_destroy(mg_sim* sim);

/* Scatter rows of `src` (same layout as the bound buffer) into the bound
 * buffer for the actor indices idx[0..n) (int32, global actor ids). */
int mg_set_indexed(mg_sim* sim, int32_t which, const float* src, const int32_t* idx, int32_t n, void* stream);

/* Reference jit functions, one thread per env. Inputs/outputs as in the
 * reference signatures; `root_states` etc. may alias the sim buffers. */
int mg_compute_observations(const mg_task_params* tp, int32_t n, const float* root_states, const float* dof_state,
                            const float* dof_force, const float* sensors, const float* actions,
                            float* potentials, float* prev_potentials, float* up_vec, float* heading_vec,
                            float* obs, void* stream);
int mg_compute_reward(const mg_task_params* tp, int32_t n, const float* obs, const float* actions,
                      const float* potentials, const float* prev_potentials, const int64_t* progress,
                      int64_t* reset, float* rew, void* stream);

/* Task-layer half of VecTask.step before the physics (pre_physics_step after the action
 * clamp): locomotion -> dof_actuation = clamp(a) * gear * power_scale (ant.py:281-285);
 * ShadowHand -> masked goal/env resets + PD targets into views->dof_targets
 * (shadow_hand.py:670-698).  sim == NULL: `views` are used. */
int mg_pre_physics(mg_sim* sim, const mg_task_params* tp, const mg_state_views* views,
                   const mg_task_buffers* tb, int32_t n, void* stream);

/* Task-layer half of VecTask.step after the physics (post_physics_step +
 * timeout + obs clamp).  With `sim`==NULL the state views in `views` are used
 * as the post-physics state (physics-free replay, parity tests). */
int mg_post_physics(mg_sim* sim, const mg_task_params* tp, const mg_state_views* views,
                    const mg_task_buffers* tb, int32_t n, void* stream);

/* ShadowHand: apply the consecutive_successes running mean (shadow_hand.py:795-798) from the partial
 * sums in tb->reduce_scratch and clear them.  Only needed with tb->defer_finalize (multi-GPU: the caller
 * all-reduces reduce_scratch over the ranks first, so every rank holds the whole-node mean). */
int mg_hand_finalize(const mg_task_params* tp, const mg_task_buffers* tb, void* stream);

/* reset_idx(env_ids) applied immediately (ant.py:252-279, humanoid.py:251-278, cartpole.py:122-136,
 * shadow_hand.py:586-668): for the n ids in `ids` (int32 device array; locomotion / MA: actor rows of
 * reset_buf, ShadowHand: envs), write the reset DOF state (noise), root row, potentials (locomotion) or
 * goal, object pose, hand DOFs and PD targets (ShadowHand), and clear progress / reset / successes --
 * the state a caller reads right after the reference's reset_idx.  Noise: the counter RNG on its own
 * stream (seed, global env id, tb->step_counter | 2^62), or tb->noise rows indexed like the step's.
 * The fused step keeps applying reset_buf's masked resets itself; this entry serves callers that reset
 * outside the step (evaluation, curricula). */
int mg_reset_idx(mg_sim* sim, const mg_task_params* tp, const mg_task_buffers* tb, const int32_t* ids, int32_t n,
                 void* stream);

/* Whole VecTask.step: actions -> actuation -> simulate -> post_physics.  Launches of one sim must be
 * stream-ordered: the multi-wave kernel instances dequeue work items from the sim's device counters,
 * which the last wave of each launch zeroes for the next. */
int mg_env_step(mg_sim* sim, const mg_task_params* tp, const mg_task_buffers* tb, void* stream);

/* Physics-bypass replay of mg_env_step (test infrastructure: pins the fused kernels' own task layer
 * to the reference's fake-gym traces).  The kernel instance mg_env_step launches is
 * run with its whole task layer (action clamp, actuation / PD targets, masked resets, observations,
 * reward, running mean, write-back), but gym.simulate is replaced by the state given here, exactly
 * as the traces' fake gym.simulate overwrites the sim state (tests/golden/make_traces.py). */
typedef struct mg_replay {
  const float* root_states;       /* (N*A*R, 13) post-simulate root rows; hand tasks (R = 3): the object
                                   * row is taken (hand and goal actors are not simulated) */
  const float* dof_state;         /* (N*A*nD, 2) */
  const float* sensors;           /* (N*A*S, 6) or NULL (zeros) */
  const float* dof_force;         /* (N*A*nD) or NULL (zeros) */
  const float* rigid_body_states; /* hand tasks: (N, nB + 2, 13); the articulation rows are taken */
  float* pre_root_states;         /* out or NULL: root rows after pre_physics_step (what simulate starts from) */
  float* pre_dof_state;           /* out or NULL: DOF state after pre_physics_step */
} mg_replay;
int mg_env_step_replay(mg_sim* sim, const mg_task_params* tp, const mg_task_buffers* tb, const mg_replay* rp,
                       void* stream);

/* ---- dynamics tensors and operational-space control (fixed-base articulations) ----
 * gym.acquire_jacobian_tensor / acquire_mass_matrix_tensor (+ refresh_*): franka_reach_MA.py:564-565, 891-911.
 * Fixed-base models only: all three calls return MG_EINVAL for a free-base model (gym's floating-base tensors
 * carry six base columns whose convention is a separate decision, out of scope here), and for a model with a free
 * object (hand tasks: three root rows per env).  DOF j is node j + 1;
 * PhysX parity of the values is not pinned: the kernels are held to the fp64 oracle. */
typedef struct mg_dynamics_views {
  float* jacobian;     /* (N*A, nB-1, 6, nD): row b-1 = body b (the fixed base link has no row, as gym);
                          [linear(3); angular(3)] of the body ORIGIN, world frame; or NULL */
  float* mass_matrix;  /* (N*A, nD, nD): joint-space inertia H(q) + diag(armature); no implicit damping or
                          stiffness terms; symmetric, both triangles written; or NULL */
} mg_dynamics_views;
int mg_dynamics_bind(mg_sim* sim, const mg_dynamics_views* views);
/* one launch: both bound tensors from the bound root_states / dof_state (and env_props, when bound: the masses
 * and armatures of the actor that is simulated) */
int mg_dynamics_refresh(mg_sim* sim, void* stream);

/* FrankaReachMA._compute_osc_torques (franka_reach_MA.py:770-802) as one launch, per actor:
 *   A = J M^-1 J^T (6 x 6), u = J^T A^-1 (kp * dpose - kd * eef_vel),
 *   u_null = kd_null * (-qd) + kp_null * wrap(default_dof_pos - q), wrap(x) = ((x + pi) mod 2 pi) - pi (floor-mod),
 *   u += (I - J^T A^-1 J M^-1) M u_null, evaluated as M u_null - J^T A^-1 J u_null (equal algebraically, no M^-1),
 *   out = clamp(u, -effort_limit, effort_limit)
 * with M the leading arm_dofs block of the full tree's mass matrix (the gripper's inertia included) and J the
 * arm_dofs leading columns of body jac_body's Jacobian rows, both computed in the kernel from the bound state (no J
 * or M goes through memory) unless jac_in / mm_in inject them.  M and A are factored by Cholesky, in double on the
 * fp32 inputs (the torques are rounded to fp32: the solve itself loses no digits to cond(A)); an actor whose
 * factorisation fails gets exactly 0 in every written column, never NaN or a garbage torque, and no other actor is
 * affected.  A factorisation fails when a pivot s_j = X_jj - sum_k L_jk^2 (X = M or A) is not above 4.4e-5 X_jj: a
 * singular or indefinite M (a massless model, a non-positive diagonal entry, a NaN), and any A that is singular to
 * working precision -- a singular pose, a J with a zero or repeated row, and every call with arm_dofs < 6 (J then
 * has rank < 6 and A is structurally singular: such calls return zeros).  The threshold is relative because
 * the fp32 pivot of a singular matrix has a random sign; it sits 13 x above the largest spurious ratio measured on
 * singular A and 13 x below the smallest true pivot ratio of the well-posed test poses (DESIGN.md s. 10). */
typedef struct mg_osc_args {
  int32_t arm_dofs;          /* 1..7: the leading DOFs that are controlled */
  int32_t jac_body;          /* body whose Jacobian rows are used (1 <= jac_body < nB) */
  const float* dpose;        /* (n, 6) */
  const float* eef_vel;      /* 6 floats per actor [linear; angular], eef_vel_stride floats apart: a contiguous
                              * (n, 6) tensor (stride 6) or columns 7:13 of a body in rigid_body_states (stride 13 nB) */
  int64_t eef_vel_stride;
  float kp[6], kd[6];
  float kp_null[7], kd_null[7];
  float default_dof_pos[7];
  float effort_limit[7];     /* +inf = no clamp */
  float* out;                /* the first out_cols torques of actor a at out + a * out_stride */
  int64_t out_stride;        /* out = dof_actuation, out_stride = nD fuses the write into the actuation tensor */
  int32_t out_cols;          /* 1..arm_dofs (the reference writes columns :6, franka_reach_MA.py:817) */
  int32_t pad_osc;
  const float* jac_in;       /* (n, 6, arm_dofs) or NULL: both given or both NULL */
  const float* mm_in;        /* (n, arm_dofs, arm_dofs) or NULL */
} mg_osc_args;
int mg_osc_torques(mg_sim* sim, const mg_osc_args* args, void* stream);
size_t mg_osc_args_sizeof(void);

/* ---- FrankaReachMA (franka_reach_MA.py): the multi-arm OSC reach task as three launches per control step --
 * mg_reach_pre, mg_sim_simulate x controlFrequencyInv, mg_reach_post -- all asynchronous on the caller's stream.
 * A arms per env (independent fixed-base articulations, actor = env * A + agent) and T <= A target cubes per env; the
 * cubes are task-owned state that only a reset moves (the reference masks them out of arm collisions and switches
 * their gravity off, franka_reach_MA.py:287, 363, 384).  New structs only: the step kernels and their argument
 * structs are untouched, and mg_task_buffers is reused for the VecTask buffers. */
typedef struct mg_reach_params {
  int32_t num_agents;          /* A: 1..MG_MAX_AGENTS */
  int32_t num_targets;         /* T: 1..A */
  int32_t num_obs;             /* 10 + 3 T + 3 (A - 1) */
  int32_t max_episode_length;
  float clip_actions, clip_obs;
  float action_scale;          /* dpose = (clamp(a) * cmd_limit) / action_scale (franka_reach_MA.py:812) */
  float cmd_limit[6];
  /* the OSC gains, null-space defaults and effort limits, as mg_osc_args carries them */
  float kp[6], kd[6];
  float kp_null[7], kd_null[7];
  float osc_default_dof_pos[7];
  float effort_limit[7];
  int32_t jac_body;            /* panda_hand: the body whose Jacobian rows drive the controller */
  int32_t eef_body;            /* panda_grip_site: the end effector (observations, eef_vel) */
  int32_t hand_body;           /* panda_hand: the net_contact_forces row of the -10 punishment */
  int32_t num_bodies;          /* rigid-body rows per arm */
  int32_t num_dofs;            /* DOFs per arm (9: 7 arm joints, 2 fingers) */
  float default_dof_pos[9];    /* franka_default_dof_pos */
  float dof_lower[9], dof_upper[9];
  float dof_noise_scale;       /* frankaDofNoise * 2.0 (the reference multiplies the Python floats first) */
  float cube_xy_center[2];     /* _table_surface_pos[:2] */
  float cube_xy_scale;         /* 2.0 * startPositionNoise */
  float cube_z_base;           /* _table_surface_pos[2] + cubeA_size / 2, summed in fp32 as the reference's tensors */
  float cube_z_range;          /* rand_z_range (0.5) */
} mg_reach_params;

/* task-owned device tensors */
typedef struct mg_reach_views {
  float* cube_states;          /* (N, T, 13) _cubeA_state */
  float* init_cube_states;     /* (N, T, 13) _init_cubeA_state */
  float* dof_targets;          /* (N*A*nD) _pos_control: the buffer the sim has bound as dof_targets */
  float* dof_actuation;        /* (N*A*nD) _effort_control: the buffer the sim has bound as dof_actuation */
} mg_reach_views;
size_t mg_reach_params_sizeof(void);
size_t mg_reach_views_sizeof(void);

/* mg_task_buffers fields the reach entry points use: actions (N*A, 6), actions_out, obs, obs_clamped, rew, reset,
 * progress, timeout, noise, seed, step_counter, env_offset, out_pack.  noise: (N, 3 T + 9) U(0,1) per env, in the
 * reference's draw order [z of each cube (T) | xy of each cube (2 T) | DOF noise (9)] (franka_reach_MA.py:692, 696,
 * 631); NULL = the counter RNG keyed by (seed, env_offset + env, step_counter, column). */

/* pre_physics_step (franka_reach_MA.py:804-819), one launch, per arm: actions_out = clamp(actions, +-clip_actions),
 * dpose = (actions_out * cmd_limit) / action_scale, the OSC torques of mg_osc_torques (J of jac_body, the leading
 * 7 x 7 of the full tree's M, eef_vel read in place from columns 7:13 of eef_body's row of the bound
 * rigid_body_states, clamped to effort_limit) written into columns 0..5 of the arm's dof_actuation row: the reference
 * writes _arm_control[:, :6], so joint 7's entry stays what the last reset left (0).  An arm whose factorisation fails
 * gets zeros (mg_osc_torques's contract). */
int mg_reach_pre(mg_sim* sim, const mg_reach_params* rp, const mg_reach_views* views, const mg_task_buffers* tb,
                 void* stream);

/* post_physics_step + the VecTask.step tail (franka_reach_MA.py:821-829, 616-679; vec_task.py step tail), one launch,
 * per env: progress += 1; the env resets when all A agents have reset != 0 (cubes, DOF state, targets, actuation,
 * progress and reset cleared; the same 9 DOF draws go to every arm); observations [cube positions 3 T | eef_quat 4 |
 * eef_pos 3 | nearest cube - eef 3 | the other agents' eef_pos, cyclic 3 (A - 1)] with the eef taken from
 * rigid_body_states as simulate left it (not recomputed after a reset: gym refreshes that tensor in simulate only);
 * compute_franka_reward; reset = 1 at progress >= max_episode_length - 1; timeout, obs clamp, out_pack.
 * state: NULL = the sim's bound views; else its dof_state, rigid_body_states and net_contact_forces are taken as the
 * post-simulate state (physics-free replay; dof_state is written by a reset). */
int mg_reach_post(mg_sim* sim, const mg_reach_params* rp, const mg_reach_views* views, const mg_task_buffers* tb,
                  const mg_state_views* state, void* stream);

/* reset_idx(agent_ids) now (franka_reach_MA.py:616-679): the envs the AND filter of the n agent ids selects
 * (bincount(ids // A) >= A: a repeated id counts twice) get the reset of mg_reach_post.  Noise: tb->noise rows by env,
 * or the counter RNG on the manual-reset stream (step_counter | 2^62), as mg_reset_idx. */
int mg_reach_reset_idx(mg_sim* sim, const mg_reach_params* rp, const mg_reach_views* views,
                       const mg_task_buffers* tb, const int32_t* ids, int32_t n, void* stream);

/* ---- Anymal (anymal.py): the PD-driven quadruped as three launches per control step -- mg_anymal_pre,
 * mg_sim_simulate x controlFrequencyInv, mg_anymal_post -- all asynchronous on the caller's stream, no host
 * synchronisation.  One free-base 12-DOF articulation per env, every DOF on a position drive (the model's drive_kp /
 * damping / effort_limit); the sim must have dof_targets, dof_force and net_contact_forces bound.  New structs only:
 * the step kernels and their argument structs are untouched, and mg_task_buffers is reused for the VecTask buffers. */
#define MG_ANYMAL_DOFS 12
#define MG_ANYMAL_OBS 48
#define MG_ANYMAL_NOISE_COLS 27
typedef struct mg_anymal_params {
  float lin_vel_scale, ang_vel_scale, dof_pos_scale, dof_vel_scale;   /* learn.*Scale (anymal.py:49-52) */
  float action_scale;                 /* control.actionScale */
  /* learn.*RewardScale * dt, the product taken in double on the host (anymal.py:99-100) and rounded to fp32 */
  float rew_lin_vel_xy, rew_ang_vel_z, rew_torque;
  float default_dof_pos[MG_ANYMAL_DOFS];   /* defaultJointAngles in DOF order */
  float base_init_state[13];          /* pos 3 | rot 4 (xyzw) | vLinear 3 | vAngular 3 */
  /* randomCommandVelocityRanges linear_x, linear_y, yaw: a draw is command_span * u + command_lo with
   * command_span = hi - lo subtracted in double on the host (torch_rand_float's Python floats) */
  float command_lo[3], command_span[3];
  int32_t base_body;                  /* net_contact_forces row of the base */
  int32_t knee_body[4];               /* ... of the four THIGH bodies */
  int32_t num_bodies;                 /* rigid-body rows per env */
  float clip_actions, clip_obs;
  int32_t max_episode_length;         /* int(episodeLength_s / dt + 0.5) */
} mg_anymal_params;

/* task-owned device tensors */
typedef struct mg_anymal_views {
  float* commands;                    /* (N, 3) [x, y, yaw] */
  float* dof_targets;                 /* (N*12): the buffer the sim has bound as dof_targets */
} mg_anymal_views;
size_t mg_anymal_params_sizeof(void);
size_t mg_anymal_views_sizeof(void);

/* mg_task_buffers fields the Anymal entry points use: actions (N, 12), actions_out, obs (N, 48), obs_clamped, rew,
 * reset, progress, timeout, noise, seed, step_counter, env_offset, out_pack.  noise: (N, 27) U(0,1) per env, in the
 * reference's draw order [positions_offset 12 | velocities 12 | command x | y | yaw] (anymal.py:283-301); NULL = the
 * counter RNG keyed by (seed, env_offset + env, step_counter, column). */

/* pre_physics_step (anymal.py:226-229), one launch: actions_out = clamp(actions, +-clip_actions), dof_targets =
 * action_scale * actions_out + default_dof_pos (a product, then a sum: no FMA). */
int mg_anymal_pre(mg_sim* sim, const mg_anymal_params* ap, const mg_anymal_views* views, const mg_task_buffers* tb,
                  void* stream);

/* post_physics_step + the VecTask.step tail (anymal.py:231-304, 311-386), one launch, per env: progress += 1; an env
 * with reset != 0 is reset (dof_pos = default * U(0.5, 1.5), dof_vel = U(-0.1, 0.1), root row = base_init_state, three
 * new commands, progress = 0), visible at once; observations [base lin vel 3 | base ang vel 3 | projected gravity 3 |
 * scaled commands 3 | dof pos 12 | dof vel 12 | actions 12]; compute_anymal_reward (clipped at 0; reset on a base or
 * THIGH net contact force norm > 1 or progress >= max_episode_length - 1) with dof_force and net_contact_forces as
 * simulate left them; timeout, obs clamp, out_pack.
 * state: NULL = the sim's bound views; else its root_states, dof_state, dof_force and net_contact_forces are taken as
 * the post-simulate state (physics-free replay; root_states and dof_state are written by a reset). */
int mg_anymal_post(mg_sim* sim, const mg_anymal_params* ap, const mg_anymal_views* views, const mg_task_buffers* tb,
                   const mg_state_views* state, void* stream);

/* reset_idx(env_ids) now (anymal.py:278-304): the n listed envs get the reset of mg_anymal_post and, as the
 * reference's reset_idx leaves them, progress = 0 and reset = 1; a repeated id is harmless, an id outside 0..N-1 is
 * skipped.  Noise: tb->noise rows by env, or the counter RNG on the manual-reset stream (step_counter | 2^62), as
 * mg_reset_idx. */
int mg_anymal_reset_idx(mg_sim* sim, const mg_anymal_params* ap, const mg_anymal_views* views,
                        const mg_task_buffers* tb, const int32_t* ids, int32_t n, void* stream);

/* ---- Quadcopter (quadcopter.py): the thrust-driven quadcopter as three launches per control step --
 * mg_quadcopter_pre, mg_sim_simulate x controlFrequencyInv with link forces on (mg_sim_set_link_forces), and
 * mg_quadcopter_post -- all asynchronous on the caller's stream, no host synchronisation, no atomics.  One free-base
 * 8-DOF, 9-body articulation per env (migym.model.quadcopter_model), every DOF on a position drive; the sim must have
 * dof_targets and rb_forces bound (MG_LOCAL_SPACE).  New structs only; mg_task_buffers is reused for the VecTask
 * buffers. */
#define MG_QUAD_DOFS 8
#define MG_QUAD_BODIES 9
#define MG_QUAD_OBS 21
#define MG_QUAD_ACTIONS 12
#define MG_QUAD_NOISE_COLS 11
typedef struct mg_quadcopter_params {
  /* dt * 8 pi and dt * 200 (quadcopter.py:310-315), each product taken in double on the host (dt the C float that
   * gymapi.SimParams.dt is) and rounded to fp32 once, as a Python float times a tensor is */
  float dof_step, thrust_step;
  float dof_lower[MG_QUAD_DOFS], dof_upper[MG_QUAD_DOFS];
  float thrust_lower, thrust_upper;           /* 0 and max_thrust = 2 (quadcopter.py:87-89) */
  float init_root[13];                        /* initial_root_states row */
  float init_dof[2 * MG_QUAD_DOFS];           /* initial_dof_states row: (pos, vel) per DOF */
  float clip_actions, clip_obs;
  int32_t max_episode_length;
  int32_t rotor_body[4];                      /* rows of the force tensor that carry the thrusts (2, 4, 6, 8) */
} mg_quadcopter_params;

/* task-owned device tensors */
typedef struct mg_quadcopter_views {
  float* thrusts;                             /* (N, 4) */
  float* dof_targets;                         /* (N*8): the buffer the sim has bound as dof_targets */
  float* forces;                              /* (N, 9, 3): the buffer the sim has bound as rb_forces */
} mg_quadcopter_views;
size_t mg_quadcopter_params_sizeof(void);
size_t mg_quadcopter_views_sizeof(void);

/* mg_task_buffers fields the Quadcopter entry points use: actions (N, 12), actions_out, obs (N, 21), obs_clamped, rew,
 * reset, progress, timeout, noise, seed, step_counter, env_offset, out_pack.  noise: (N, 11) U(0,1) per env in the
 * reference's draw order [x | y | z | dof position 8] (quadcopter.py:289-294), mapped as torch_rand_float does,
 * (upper - lower) * u + lower; NULL = the counter RNG keyed by (seed, env_offset + env, step_counter, column). */

/* pre_physics_step (quadcopter.py:301-330), one launch, per env, in the reference's order: an env with reset != 0 is
 * reset first (DOF state and root row from the initial state, x, y += U(-1.5, 1.5), z += U(-0.2, 1.5), DOF positions
 * U(-0.2, 0.2), velocities 0, reset = 0, progress = 0); actions_out = clamp(actions, +-clip_actions); targets +=
 * dof_step * a[0:8], clamped to the DOF limits; thrusts += thrust_step * a[8:12], clamped to [thrust_lower,
 * thrust_upper]; forces[rotor_body[k]][2] = thrusts[k]; for the envs just reset thrusts = 0, their force rows = 0 and
 * targets = the new DOF positions.  Products, then sums: no FMA. */
int mg_quadcopter_pre(mg_sim* sim, const mg_quadcopter_params* qp, const mg_quadcopter_views* views,
                      const mg_task_buffers* tb, void* stream);

/* post_physics_step + the VecTask.step tail (quadcopter.py:332-418), one launch, per env: progress += 1;
 * observations [(target - pos) / 3 | quat | linvel / 2 | angvel / pi | dof pos], target (0, 0, 1);
 * compute_quadcopter_reward (reset on target_dist > 3, z < 0.3, or progress >= max_episode_length - 1); timeout, the
 * observation clamp, out_pack.  state: NULL = the sim's bound views; else its root_states and dof_state are taken as the
 * post-simulate state (physics-free replay). */
int mg_quadcopter_post(mg_sim* sim, const mg_quadcopter_params* qp, const mg_quadcopter_views* views,
                       const mg_task_buffers* tb, const mg_state_views* state, void* stream);

/* reset_idx(env_ids) now (quadcopter.py:280-299): the n listed envs get the state reset of mg_quadcopter_pre (not its
 * clearing of thrusts, forces and targets, which pre_physics_step does), reset = 0 and progress = 0; a repeated id
 * writes the same values twice, an id outside 0..N-1 is skipped.  Noise: tb->noise rows by env, or the counter RNG on
 * the manual-reset stream (step_counter | 2^62), as mg_reset_idx. */
int mg_quadcopter_reset_idx(mg_sim* sim, const mg_quadcopter_params* qp, const mg_quadcopter_views* views,
                            const mg_task_buffers* tb, const int32_t* ids, int32_t n, void* stream);

/* ---- Rendering (VecTask.render under virtual_screen_capture, tasks/base/vec_task.py render): a pinhole ray caster
 * over the envs' collision geometry, two launches on the caller's stream, no host synchronisation.  The image shows
 * the model's geoms, the hand tasks' free object and goal, the caller's extra boxes and the ground plane z = 0; visual
 * meshes, textures and shadows are not drawn.  Additive: no existing struct or export changes.
 *   camera     f = normalize(target - eye), r = normalize(f x (0,0,1)), u = r x f;
 *              eye = anchor + eye_offset, target = anchor + target_offset, anchor = the root position of the env's
 *              actor 0 when follow != 0, else the origin
 *   pixel      (row i, column j): x = (2 (j + 0.5) / W - 1) tan(fov_y / 2) W / H, y = (1 - 2 (i + 0.5) / H) tan(fov_y / 2),
 *              d = normalize(f + x r + y u); the nearest hit with t > 1e-4 wins, a tie goes to the lower primitive id
 *   primitives of an env, in id order: the geoms 0..nG-1 of each actor a = 0..A-1; the free object and the goal (root
 *              rows 1 and 2 of the env, shaped by obj_type / obj_size) when obj_type != 0; the num_boxes extra boxes;
 *              the ground plane, last.  P = A nG + (obj_type ? 2 : 0) + num_boxes + 1 <= 512 (else MG_ECAPACITY)
 *   shading    c = base (0.35 + 0.65 max(0, n . l)), l = normalize(0.3, 0.2, 1), n the outward world normal; base = an
 *              8-entry palette indexed by geom_body % 8, fixed colours for the object, the goal and the extra boxes, a
 *              two-grey 1 m checker ((floor(x) + floor(y)) & 1) on the ground, one sky colour;
 *              uint8 = clamp(floor(255 c + 0.5), 0, 255)
 * An env id outside 0..N-1 in the device list env_ids cannot be reported (nothing synchronises): its image is sky,
 * depth +inf, ids -1.  migym/render.py checks ids it is given as a host list. */
typedef struct mg_render_args {
  int32_t width, height;       /* 1..16384 each */
  float fov_y;                 /* vertical field of view, radians, in (0, pi) */
  float eye_offset[3];
  float target_offset[3];
  int32_t follow;
  const int32_t* env_ids;      /* (n_sel) device, or NULL = the first n_sel envs */
  int32_t n_sel;               /* >= 1 */
  int32_t num_boxes;           /* K >= 0 */
  const float* boxes;          /* (N, K, 10) device: pos 3, quat xyzw 4, half extents 3, indexed by env id; NULL if K == 0 */
  float* scratch;              /* mg_render_scratch_floats() floats, 16-byte aligned: (n_sel, P, 16) primitive records
                                * [world rotation 9 row-major | world position 3 | size 3 | type + (colour << 8)] */
  uint8_t* rgb;                /* (n_sel, H, W, 3) or NULL */
  float* depth;                /* (n_sel, H, W): t along the unit ray, +inf for sky; or NULL */
  int32_t* ids;                /* (n_sel, H, W): primitive id, -1 for sky; or NULL.  Not all three NULL */
} mg_render_args;
size_t mg_render_args_sizeof(void);
/* floats of scratch for n_sel envs and num_boxes extra boxes; 0 for bad arguments or more than 512 primitives */
size_t mg_render_scratch_floats(const mg_sim* sim, int32_t n_sel, int32_t num_boxes);
/* MG_EINVAL (and nothing is launched or written) for: a size or fov out of range, eye == target or a view along z,
 * all outputs NULL, n_sel < 1 (or > N with env_ids NULL), num_boxes < 0 or boxes NULL with num_boxes > 0, a NULL or
 * misaligned scratch, a sim whose state is not bound. */
int mg_render(mg_sim* sim, const mg_render_args* args, void* stream);

/* ---- HumanoidAMP (humanoid_amp.py, amp/humanoid_amp_base.py, amp/utils_amp/motion_lib.py): the AMP humanoid as three
 * launches per control step -- mg_amp_pre, mg_sim_simulate x controlFrequencyInv, mg_amp_post -- plus mg_amp_reset_idx
 * (reset_idx(env_ids), all four StateInit modes, sampled from a device motion table) and mg_amp_obs_demo
 * (fetch_amp_obs_demo).  All asynchronous on the caller's stream, no host synchronisation, no atomics.  One free-base
 * 28-DOF, 15-body articulation per env; the sim must have rigid_body_states and net_contact_forces bound, and
 * dof_targets (pd_control) or dof_actuation (effort mode).  New structs only; mg_task_buffers is reused. */
#define MG_AMP_DOFS 28
#define MG_AMP_BODIES 15
#define MG_AMP_OBS 105          /* root_h 1 | root rot 6 | root vel 3 | root ang vel 3 | dof obs 52 | dof vel 28 | key 12 */
#define MG_AMP_KEY_BODIES 4
#define MG_AMP_FRAME_FLOATS 113 /* one motion frame, see mg_amp_views.motion_frames */
#define MG_AMP_MAX_OBS_STEPS 16 /* numAMPObsSteps: 2 .. 16 */
#define MG_AMP_NOISE_COLS 3     /* reset noise row [hybrid | motion | phase] */
#define MG_AMP_INIT_DEFAULT 0
#define MG_AMP_INIT_START 1
#define MG_AMP_INIT_RANDOM 2
#define MG_AMP_INIT_HYBRID 3
typedef struct mg_amp_params {
  /* _build_pd_action_offset_scale (humanoid_amp_base.py:262-295), computed in double on the host, rounded once */
  float pd_action_offset[MG_AMP_DOFS], pd_action_scale[MG_AMP_DOFS];
  float motor_effort[MG_AMP_DOFS];     /* actuator gears (effort mode: a * motor_effort * power_scale) */
  float initial_dof_pos[MG_AMP_DOFS];  /* zero but right_shoulder_x = pi/2, left_shoulder_x = -pi/2 */
  float initial_root[13];              /* z = 0.89, identity rotation, zero twist */
  double dt;                           /* controlFrequencyInv * sim.dt, a Python double (humanoid_amp_base.py:75-76) */
  float power_scale;
  float termination_height;
  float hybrid_init_prob;
  float clip_actions, clip_obs;
  int32_t max_episode_length;
  int32_t enable_early_termination, local_root_obs, pd_control;
  int32_t state_init;                  /* MG_AMP_INIT_* */
  int32_t num_amp_obs_steps;
  int32_t key_body[MG_AMP_KEY_BODIES]; /* right_hand, left_hand, right_foot, left_foot */
  uint32_t contact_body_mask;          /* bit b: body b is one of env.contactBodies */
  int32_t num_bodies;                  /* rigid-body rows per env (15) */
} mg_amp_params;

/* task-owned device tensors and the motion table (migym/motion.py) */
typedef struct mg_amp_views {
  float* dof_targets;        /* (N*28): the buffer the sim has bound as dof_targets (pd_control) */
  float* dof_actuation;      /* (N*28): the buffer the sim has bound as dof_actuation (effort mode) */
  float* amp_obs;            /* (N, num_amp_obs_steps, 105): slot 0 the current step, slot k the k-th before */
  int64_t* terminate;        /* (N) _terminate_buf */
  /* (F, 113) fp32, the frames of all motions back to back: root pos 3 | root rot 4 (xyzw) | root vel 3 | root ang
   * vel 3 | local rotations 15 x 4 | dof vel 28 | key-body positions 4 x 3 */
  const float* motion_frames;
  const int32_t* motion_index;  /* (M, 2): first frame, frame count (>= 2) */
  const double* motion_time;    /* (M, 3): frame dt, length = dt * (frames - 1), cumulative normalised weight */
  int32_t num_motions;          /* M >= 1 */
  int32_t num_frames;           /* F */
} mg_amp_views;
size_t mg_amp_params_sizeof(void);
size_t mg_amp_views_sizeof(void);

/* pre_physics_step (humanoid_amp_base.py:362-374, 419-421), one launch: actions_out = clamp(actions, +-clip_actions);
 * pd_control: dof_targets = pd_action_offset + pd_action_scale * actions_out (a product, then a sum: no FMA); else
 * dof_actuation = actions_out * motor_effort * power_scale. */
int mg_amp_pre(mg_sim* sim, const mg_amp_params* ap, const mg_amp_views* views, const mg_task_buffers* tb,
               void* stream);

/* post_physics_step of both classes + the VecTask.step tail (humanoid_amp_base.py:376-390, 494-562,
 * humanoid_amp.py:87-96, 274-333), one launch, per env: progress += 1; the 105 observations of
 * compute_humanoid_observations from root_states, dof_state and the key bodies' rigid_body_states rows; reward 1;
 * compute_humanoid_reset (fallen = any signed net-contact-force component > 0.1 on a non-contact body AND any
 * non-contact body below termination_height AND progress > 1; reset = progress >= max_episode_length - 1 or
 * terminated), reset and terminate written separately; the AMP history shifted by one slot, slot 0 =
 * build_amp_observations; timeout, obs clamp, out_pack.  It resets nothing (the reference's step does not).
 * state: NULL = the sim's bound views; else its root_states, dof_state, rigid_body_states and net_contact_forces are
 * taken as the post-simulate state (physics-free replay). */
int mg_amp_post(mg_sim* sim, const mg_amp_params* ap, const mg_amp_views* views, const mg_task_buffers* tb,
                const mg_state_views* state, void* stream);

/* reset_idx(env_ids) (humanoid_amp.py:146-256), one launch, one 32-lane team per listed id.  tb->noise: (n, 3) U(0,1)
 * rows BY LIST POSITION, [hybrid | motion | phase]; NULL = the counter RNG keyed by (seed, env_offset + env,
 * step_counter | 2^62, column).  Hybrid takes the reference path when u < hybrid_init_prob; motion id = the first
 * index whose cumulative weight exceeds u; time = u * length (Start: 0).  Reference path: root row and DOF state from
 * the motion (MotionLib.get_motion_state: frame index, blend and times in fp64, lerp / slerp / exp maps in fp32,
 * velocities of frame idx0 unblended), the AMP history from the motion at t - k dt.  Default path: initial_root and
 * initial_dof_pos, the history copies of the current slot.  Both: progress = reset = terminate = 0, the env's
 * observation row and AMP slot 0 from the written root / DOF state and the rigid_body_states rows AS BOUND (not
 * refreshed: the reference reads its stale _rigid_body_pos here too).  A repeated id writes the same values twice
 * when its noise rows agree; an id outside 0..N-1 is skipped. */
int mg_amp_reset_idx(mg_sim* sim, const mg_amp_params* ap, const mg_amp_views* views, const mg_task_buffers* tb,
                     const int32_t* ids, int32_t n, void* stream);

/* fetch_amp_obs_demo(num_samples) (humanoid_amp.py:108-133): out (num_samples, num_amp_obs_steps, 105) from the
 * motion table alone; sample i draws [motion | phase] from noise (num_samples, 2), or NULL = the counter RNG keyed by
 * (seed, i, counter | 2^61, column); slot k is build_amp_observations of the motion at t - k dt.  Needs no sim. */
int mg_amp_obs_demo(const mg_amp_params* ap, const mg_amp_views* views, const float* noise, uint64_t seed,
                    uint64_t counter, float* out, int32_t num_samples, void* stream);

/* ---- AnymalTerrain (anymal_terrain.py): rough-terrain locomotion with a terrain curriculum.  A control step is
 * (mg_anymal_terrain_pre, mg_sim_simulate) x decimation, then mg_anymal_terrain_post (one launch over the envs and
 * one small finishing launch for the cross-env means), all asynchronous on the caller's stream, no host
 * synchronisation, no floating-point atomics.  One free-base 12-DOF articulation per env in effort mode; the sim must
 * have dof_actuation and net_contact_forces bound, and root_states in world coordinates (the heightfield set without
 * per-actor origins).  New structs only. */
#define MG_ANYMAL_TERRAIN_OBS 188
#define MG_ANYMAL_TERRAIN_HEIGHT_POINTS 140
#define MG_ANYMAL_TERRAIN_NOISE_COLS 219
#define MG_ANYMAL_TERRAIN_REWARDS 13
typedef struct mg_anymal_terrain_params {
  /* learn.*Scale (anymal_terrain.py:54-58) */
  float lin_vel_scale, ang_vel_scale, dof_pos_scale, dof_vel_scale, height_meas_scale;
  /* learn.*RewardScale * dt, dt = decimation * sim.dt, the product taken in double on the host and rounded to fp32
   * once (anymal_terrain.py:104-105), in the order of episode_sums: lin_vel_xy, lin_vel_z, ang_vel_z, ang_vel_xy,
   * orient, torques, joint_acc, base_height, air_time, collision, stumble, action_rate, hip */
  float rew_scale[MG_ANYMAL_TERRAIN_REWARDS];
  float rew_termination;              /* terminalReward * dt */
  float dt;                           /* what feet_air_time advances by per control step: sim.dt, not decimation *
                                       * sim.dt -- VecTask.__init__ overwrites the task's self.dt (vec_task.py:242) */
  float Kp, Kd, action_scale, torque_clip;   /* control.stiffness, damping, actionScale; 80 */
  float default_dof_pos[MG_ANYMAL_DOFS];
  float base_init_state[13];
  float command_lo[3], command_span[3];      /* linear_x, linear_y, heading (the YAML's yaw): span = hi - lo in double */
  int32_t base_body, knee_body[4], foot_body[4];   /* net_contact_forces rows */
  int32_t hip_dof[4];                 /* the DOF columns of the hip penalty (0, 3, 6, 9) */
  int32_t num_bodies;
  int32_t allow_knee_contacts, add_noise;
  float noise_scale_vec[MG_ANYMAL_TERRAIN_OBS];
  int32_t max_episode_length;         /* int(episodeLength_s / dt + 0.5) */
  float max_episode_length_s;
  float env_length;                   /* terrain.mapLength: an env climbs a level past env_length / 2 */
  int32_t env_rows, env_cols;         /* numLevels, numTerrains: the shape of terrain_origins */
  int32_t curriculum, custom_origins;
  /* the height scan's field, mg_height_scan's rule: heights[i * ny + j] in metres (vertical_scale applied) at world
   * (x0 + i dx, y0 + j dx); NULL (terrainType plane): every height 0 */
  const float* hf_heights;
  int32_t hf_nx, hf_ny;
  float hf_dx, hf_x0, hf_y0;
  float height_points[2 * MG_ANYMAL_TERRAIN_HEIGHT_POINTS];   /* (x, y) in the base's yaw frame */
  float clip_actions, clip_obs;
  int32_t pad_atp;
} mg_anymal_terrain_params;

/* task-owned device tensors */
typedef struct mg_anymal_terrain_views {
  float* commands;                    /* (N, 4) [x, y, yaw rate, heading] */
  float* torques;                     /* (N, 12) the last substep's PD torques */
  float* last_actions;                /* (N, 12) */
  float* last_dof_vel;                /* (N, 12) */
  float* feet_air_time;               /* (N, 4) */
  float* episode_sums;                /* (N, 13), columns as rew_scale */
  int32_t* terrain_levels;            /* (N) */
  const int32_t* terrain_types;       /* (N) */
  float* env_origins;                 /* (N, 3) */
  const float* terrain_origins;       /* (env_rows, env_cols, 3) */
  float* dof_actuation;               /* (N*12): the buffer the sim has bound as dof_actuation */
  float* episode_out;                 /* (14): 13 means / max_episode_length_s and the mean terrain level; written only
                                       * by a launch in which at least one env reset */
  float* measured_heights;            /* (N, 140) get_heights as the observations took it, or NULL */
  float* partials;                    /* (ceil(N / 4), 16) scratch of the two-stage means */
  int32_t* reset_mark;                /* (N) scratch of mg_anymal_terrain_reset_idx, all zero between calls */
  int32_t push_now;                   /* set by the host per step: push_robots runs in this post */
  int32_t pad_atv;
} mg_anymal_terrain_views;
size_t mg_anymal_terrain_params_sizeof(void);
size_t mg_anymal_terrain_views_sizeof(void);

/* mg_task_buffers fields these entry points use: actions (N, 12), actions_out, obs (N, 188), obs_clamped, rew, reset,
 * progress, timeout, noise, seed, step_counter, env_offset, out_pack.  noise: (N, 219) U(0,1) per env in the
 * reference's draw order [push vx vy 2 | positions_offset 12 | velocities 12 | root x y 2 | command x | y | heading |
 * observation noise 188]; NULL = the counter RNG keyed by (seed, env_offset + env, step_counter, column). */

/* The explicit PD torque of one decimation step (anymal_terrain.py:443-447), one lane per (env, DOF): a =
 * clamp(actions, +-clip_actions) -> actions_out; torque = clip(Kp * (action_scale * a + default - dof_pos) - Kd *
 * dof_vel, +-torque_clip) in the reference's operation order, no FMA -> the bound dof_actuation and views.torques.
 * Launched before every mg_sim_simulate of a control step. */
int mg_anymal_terrain_pre(mg_sim* sim, const mg_anymal_terrain_params* ap, const mg_anymal_terrain_views* views,
                          const mg_task_buffers* tb, void* stream);

/* post_physics_step + the VecTask.step tail (anymal_terrain.py:453-485, 294-436), per env and in the reference's
 * order: progress += 1; the push (views.push_now); base velocities, projected gravity, heading and commands[2] from the
 * root row; check_termination; compute_reward (timeout read as the previous step left it); the envs whose reset flag
 * was just set are reset in the same launch (curriculum by the per-env command norm, DOF draws, root row at the env
 * origin, new commands); observations (base-frame columns stale for a reset env, as in the reference), noise,
 * last_actions, last_dof_vel; timeout, the observation clamp, out_pack.  Then the finishing launch writes episode_out
 * if any env reset.  state: NULL = the sim's bound views; else its root_states, dof_state and net_contact_forces are
 * taken as the post-simulate state (root_states and dof_state are written by a push or a reset). */
int mg_anymal_terrain_post(mg_sim* sim, const mg_anymal_terrain_params* ap, const mg_anymal_terrain_views* views,
                           const mg_task_buffers* tb, const mg_state_views* state, void* stream);

/* reset_idx(env_ids) now (anymal_terrain.py:384-425): the listed envs get the reset of mg_anymal_terrain_post,
 * last_actions = last_dof_vel = 0, progress = 0 and reset = 1; update_levels != 0 runs update_terrain_level first (0:
 * the constructor's reset, the reference's init_done).  A repeated id is harmless, an id outside 0..N-1 is skipped.
 * Noise: tb->noise rows by env, or the counter RNG on the manual-reset stream (step_counter | 2^62). */
int mg_anymal_terrain_reset_idx(mg_sim* sim, const mg_anymal_terrain_params* ap,
                                const mg_anymal_terrain_views* views, const mg_task_buffers* tb, const int32_t* ids,
                                int32_t n, int32_t update_levels, void* stream);

/* Measurement aid (no reference counterpart; bench.py's roofline.kernel_ms): the device-side duration of the
 * fused step kernel, from the first wave's start to the last wave's end on the GPU's constant wall clock
 * (wall_clock64, hipDeviceAttributeWallClockRate), so that no launch, queue or event-packet overhead is in it.
 * mg_kernel_span_begin(sim, cap): the next `cap` mg_env_step launches of `sim` record their span (one slot each;
 * 0 turns recording off; the kernels run unchanged otherwise).  mg_kernel_span_read(sim, ms, cap, &n):
 * synchronises the device and returns the recorded spans in milliseconds, in launch order. */
int mg_kernel_span_begin(mg_sim* sim, int32_t cap);
int mg_kernel_span_read(mg_sim* sim, double* ms, int32_t cap, int32_t* n_out);
/* mg_kernel_span_waves(sim, launch, out, cap, &n): the raw per-wave (start, end) GPU wall-clock ticks of recorded
 * launch `launch` (out: 2 * cap uint64; n = the launch's waves, at most cap; ticks at hipDeviceAttributeWallClockRate
 * kHz) -- the launch's tail and dispatch ramp for tools/span_diag.py --waves */
int mg_kernel_span_waves(mg_sim* sim, int32_t launch, uint64_t* out, int32_t cap, int32_t* n_out);

/* Test aid (no reference counterpart): the work ordering's state.  mg_work_order(sim, order, cost,
 * cap, &mode, &n): synchronises the device; mode = 0 off, 1 lists, 2 sort; under the sort n = the env units (envs,
 * an MA env's agents counted once), `order` (n int32, or NULL) = the permutation the last mg_env_step ran in (slot ->
 * unit; the identity before the first sort) and `cost` (n uint8, or NULL) = the row counts that launch wrote (the
 * next sort's keys); at most cap entries are copied.  Off and lists report n = 0. */
int mg_work_order(mg_sim* sim, int32_t* order, uint8_t* cost, int32_t cap, int32_t* mode, int32_t* n_out);
/* Diagnostic (no reference counterpart): the step-kernel instance the dispatcher picked for `sim`:
 * team_lanes = lanes per actor (T), compact = 1 for the 12-waves-per-CU compact team layout, 0 for the classic one
 * (MIGYM_LAYOUT = auto | compact | classic, read at mg_sim_create). */
int mg_sim_kernel_layout(mg_sim* sim, int32_t* team_lanes, int32_t* compact);
/* The same rule without a sim or a device: team_lanes = lanes per actor of the first instance that fits `model` at
 * `max_contacts` contacts (mgi::team_size, csrc/dispatch.hpp), 0 if none fits.  Host code only. */
int mg_model_team_lanes(const mg_model* model, int32_t max_contacts, int32_t* team_lanes);

#ifdef __cplusplus
}
#endif
#endif /* MIGYM_H */
