"""numpy restatement of FrankaReachMA's post_physics_step and the VecTask.step tail (franka_reach_MA.py:821-829,
616-704, 519-612, 928-960; vec_task.py step tail), in float32 and the reference's operation order.

Test infrastructure: tests/test_franka_reach_host.py holds it to the reference's own output
(tests/golden/trace_franka_reach_ma.npz); the GPU tests use it where no recorded trace exists (the device RNG).

State (a dict of arrays, updated in place by ``post_step``):
  progress, reset (N*A) int64; cube, init_cube (N, T, 13); q, qd, pos_control, effort_control (N, A*9) float32.
Per-step inputs: eef (N, A, 13) the grip site's rigid-body rows as simulate left them, hand_force (N, A, 3) the
hand's net contact force rows, actions (N*A, 6) (clamped inside), noise (N, 3T+9) U(0,1) rows
[z of each cube (T) | xy of each cube (2T) | DOF noise (9)].
"""
import numpy as np

F = np.float32
DEFAULT_DOF_POS = np.array([0, 0.1963, 0, -2.6180, 0, 2.9416, 0.7854, 0.035, 0.035], F)


def params_from(rp):
    """the constants ``post_step`` reads, from a ctypes mg_reach_params (taskdefs.reach_params)"""
    return dict(A=int(rp.num_agents), T=int(rp.num_targets), max_episode_length=int(rp.max_episode_length),
                clip_actions=F(rp.clip_actions), clip_obs=F(rp.clip_obs), dof_noise_scale=F(rp.dof_noise_scale),
                cube_xy_center=np.array(list(rp.cube_xy_center), F), cube_xy_scale=F(rp.cube_xy_scale),
                cube_z_base=F(rp.cube_z_base), cube_z_range=F(rp.cube_z_range),
                default_dof_pos=np.array(list(rp.default_dof_pos), F), dof_lower=np.array(list(rp.dof_lower), F),
                dof_upper=np.array(list(rp.dof_upper), F))


def and_filter(ids, A, N):
    """_agent_ids_to_env_ids(use_AND_filter=True): envs whose ids count at least A times"""
    cnt = np.bincount(np.asarray(ids, np.int64) // A, minlength=N)[:N]
    return np.nonzero(cnt >= A)[0]


def reset_envs(p, st, env_ids, noise):
    """reset_idx for the (already filtered) envs: cubes, DOF state, controls, counters"""
    A, T = p["A"], p["T"]
    for e in env_ids:
        u = noise[e].astype(F)
        c = np.zeros((T, 13), F)
        c[:, 2] = p["cube_z_base"] + u[:T] * p["cube_z_range"]
        c[:, 0:2] = p["cube_xy_center"][None] + p["cube_xy_scale"] * (u[T:3 * T].reshape(T, 2) - F(0.5))
        c[:, 6] = 1.0
        st["init_cube"][e] = c
        st["cube"][e] = c
        pos = p["default_dof_pos"] + p["dof_noise_scale"] * (u[3 * T:3 * T + 9] - F(0.5))
        pos = np.maximum(np.minimum(pos, p["dof_upper"]), p["dof_lower"]).astype(F)
        pos[-2:] = p["default_dof_pos"][-2:]
        pos = np.tile(pos, A)
        st["q"][e] = pos
        st["qd"][e] = 0
        st["pos_control"][e] = pos
        st["effort_control"][e] = 0
        st["progress"][e * A:(e + 1) * A] = 0
        st["reset"][e * A:(e + 1) * A] = 0


def observe(p, st, eef):
    """_update_states + compute_observations: (obs (N*A, nO), nearest-cube ids (N, A), min-relative (N, A, 3))"""
    A, T = p["A"], p["T"]
    N = eef.shape[0]
    c = st["cube"][:, :, :3]
    a = eef[:, :, :3]
    rel = c[:, None, :, :] - a[:, :, None, :]                        # (N, A, T, 3)
    norm = np.sqrt((rel * rel).sum(-1, dtype=F))
    ids = np.argmin(norm, -1)                                        # first index on ties
    min_rel = np.take_along_axis(rel, ids[:, :, None, None], 2)[:, :, 0]
    all_targets = np.repeat(c.reshape(N, -1), A, 0)
    own = np.concatenate([eef[:, :, 3:7], a, min_rel], -1).reshape(N * A, -1)
    flat = a.reshape(N, -1)
    shifted = np.stack([np.concatenate([flat[:, 3 * i:], flat[:, :3 * i]], 1) for i in range(A)], 1)
    others = shifted[..., 3:].reshape(N * A, -1)
    return np.concatenate([all_targets, own, others], -1).astype(F), ids, min_rel


def reward(p, st, actions, ids, min_rel, hand_force):
    """compute_franka_reward: (rew (N*A), reset (N*A)); float32 as torch evaluates it"""
    A = p["A"]
    N = ids.shape[0]
    mr = min_rel.reshape(-1, 3)
    d = np.sqrt((mr * mr).sum(-1, dtype=F))
    r = F(1.0) / (F(0.5) + d * d) - (actions * actions).sum(-1, dtype=F) * F(0.01)
    mask = np.zeros((N, A), np.int64)
    np.put_along_axis(mask, ids, 1, 1)
    touched = np.repeat((mask.sum(-1) / A).astype(F), A)
    hf = hand_force.reshape(-1, 3)
    punish = (np.sqrt((hf * hf).sum(-1, dtype=F)) >= F(0.1)) * F(-10.0)
    r = np.maximum(r + (touched + punish), F(0.0)).astype(F)
    rst = np.where(st["progress"] >= p["max_episode_length"] - 1, 1, st["reset"])
    return r, rst


def post_step(p, st, eef, hand_force, actions, noise):
    """steps 1-6: returns dict(obs, obs_clamped, rew, timeout); st holds reset / progress and the task state"""
    A = p["A"]
    N = eef.shape[0]
    act = np.clip(actions.astype(F), -p["clip_actions"], p["clip_actions"])
    st["progress"] += 1
    done = np.nonzero(st["reset"])[0]
    if len(done):
        reset_envs(p, st, and_filter(done, A, N), noise)
    obs, ids, min_rel = observe(p, st, eef.astype(F))
    rew, st["reset"][:] = reward(p, st, act, ids, min_rel, hand_force.astype(F))
    timeout = (st["progress"] >= p["max_episode_length"] - 1) & (st["reset"] != 0)
    return dict(obs=obs, obs_clamped=np.clip(obs, -p["clip_obs"], p["clip_obs"]), rew=rew, timeout=timeout,
                nearest=ids)


# ---- the reference trace (tests/golden/trace_franka_reach_ma.npz, written by tests/golden/make_franka_reach_golden.py)
import functools  # noqa: E402
import os  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "trace_franka_reach_ma.npz")
FRANKA_JSON = os.path.join(HERE, "golden", "franka_panda.json")
STATE_KEYS = ("cube", "init_cube", "q", "qd", "pos_control", "effort_control")


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN))
    for v in g.values():
        v.setflags(write=False)
    return g


def golden_cfg(A, T, N, g=None, **env):
    """the task config the trace was generated for (env overrides on top)"""
    from migym import configs
    g = g or golden()
    over = {"env.numAgents": A, "env.numTargets": T, "env.episodeLength": int(g["max_episode_length"]),
            "env.clipActions": float(g["clip_actions"]), "env.clipObservations": float(g["clip_obs"]),
            "env.startPositionNoise": float(g["start_position_noise"]),
            "env.frankaDofNoise": float(g["franka_dof_noise"]), "env.asset": {"modelTable": FRANKA_JSON}}
    over.update({"env." + k: v for k, v in env.items()})
    return configs.task_config("FrankaReachMA", N, overrides=over)


def golden_state0(g, A, T, N):
    """the task state before step 0 (q / qd are overwritten by every step's post-simulate input)"""
    tag = f"A{A}T{T}_"
    st = {k: g[tag + k + "_0"].copy() for k in ("cube", "init_cube", "pos_control", "effort_control")}
    st["q"], st["qd"] = np.zeros((N, A * 9), F), np.zeros((N, A * 9), F)
    st["progress"], st["reset"] = np.zeros(N * A, np.int64), np.zeros(N * A, np.int64)
    return st


def reward_close(rew, ref):
    """the project's 1e-4 rule: |x - ref| <= 1e-4 max(1, |ref|)"""
    return np.abs(rew.astype(np.float64) - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))
