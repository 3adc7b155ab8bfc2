"""numpy restatement of AnymalTerrain's pre_physics_step torque, post_physics_step and the VecTask.step tail
(anymal_terrain.py:294-485, 515-538; vec_task.py step tail), in float32 and the reference's operation order, with the
helpers the AnymalTerrain tests share: the reference trace, the config it was generated for, the synthetic terrain.

Test infrastructure: tests/test_anymal_terrain_host.py holds the restatement to the reference's own output
(tests/golden/trace_anymal_terrain.npz); the GPU tests use it where no recorded trace exists (the device RNG).

State (a dict of arrays, updated in place by ``post_step``): progress, reset (N) int64, timeout (N) bool; root (N, 13),
dof (N, 12, 2), commands (N, 4), torques, last_actions, last_dof_vel (N, 12), feet_air_time (N, 4), episode_sums
(N, 13), env_origins (N, 3) float32; terrain_levels, terrain_types (N) int32; episode_out (14) float32.
Per-step inputs: ncf (N, nB, 3), actions (N, 12) (clamped inside), noise (N, 219) U(0,1) rows [push 2 |
positions_offset 12 | velocities 12 | root x y 2 | command x | y | heading | observation noise 188], push_now.
"""
import functools
import os

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "trace_anymal_terrain.npz")
LAYOUT = os.path.join(HERE, "golden", "terrain_layout.npz")
ANYMAL_JSON = os.path.join(HERE, "golden", "anymal_c.json")
COLS = 219
CLIP_ACTIONS, CLIP_OBS = 1.0, 5.0   # the trace's: the reference's YAML sets neither
C_PUSH, C_POS, C_VEL, C_ROOT, C_CMD, C_OBS = 0, 2, 14, 26, 28, 31
STATE_KEYS = ("progress", "reset", "timeout", "root", "dof", "commands", "torques", "last_actions", "last_dof_vel",
              "feet_air_time", "episode_sums", "env_origins", "terrain_levels", "terrain_types", "episode_out")


def params_from(ap, table=None, terrain_origins=None):
    """the constants the restatement reads, from a ctypes mg_anymal_terrain_params (taskdefs.anymal_terrain_params);
    table: the scan's field in metres (nx, ny) or None (plane); terrain_origins (rows, cols, 3)"""
    return dict(lin=F(ap.lin_vel_scale), ang=F(ap.ang_vel_scale), dof_pos=F(ap.dof_pos_scale),
                dof_vel=F(ap.dof_vel_scale), hscale=F(ap.height_meas_scale), rew=np.array(list(ap.rew_scale), F),
                rew_term=F(ap.rew_termination), dt=F(ap.dt), Kp=F(ap.Kp), Kd=F(ap.Kd),
                action_scale=F(ap.action_scale), torque_clip=F(ap.torque_clip),
                default=np.array(list(ap.default_dof_pos), F), base_init=np.array(list(ap.base_init_state), F),
                cmd_lo=np.array(list(ap.command_lo), F), cmd_span=np.array(list(ap.command_span), F),
                base=int(ap.base_body), knees=list(ap.knee_body), feet=list(ap.foot_body), hips=list(ap.hip_dof),
                allow_knee=bool(ap.allow_knee_contacts), add_noise=bool(ap.add_noise),
                noise_vec=np.array(list(ap.noise_scale_vec), F), max_episode_length=int(ap.max_episode_length),
                max_s=F(ap.max_episode_length_s), env_length=F(ap.env_length), env_rows=int(ap.env_rows),
                curriculum=bool(ap.curriculum), custom_origins=bool(ap.custom_origins), table=table,
                dx=F(ap.hf_dx), x0=F(ap.hf_x0), y0=F(ap.hf_y0), terrain_origins=terrain_origins,
                points=np.array(list(ap.height_points), F).reshape(-1, 2), clip_actions=F(ap.clip_actions),
                clip_obs=F(ap.clip_obs))


def pre_step(p, actions, dof):
    """(actions_out, torques): clip(Kp * (action_scale * a + default - dof_pos) - Kd * dof_vel, -80, 80), one rounding
    per operation"""
    a = np.clip(actions.astype(F), -p["clip_actions"], p["clip_actions"])
    t = ((p["action_scale"] * a).astype(F) + p["default"][None]).astype(F)
    t = (t - dof[..., 0]).astype(F)
    t = ((p["Kp"] * t).astype(F) - (p["Kd"] * dof[..., 1]).astype(F)).astype(F)
    return a, np.clip(t, -p["torque_clip"], p["torque_clip"]).astype(F)


def quat_rotate_inverse(q, v):
    qw, qv = q[:, 3:4], q[:, :3]
    a = v * (F(2.0) * qw * qw - F(1.0))
    b = np.cross(qv, v).astype(F) * qw * F(2.0)
    c = qv * (qv * v).sum(-1, dtype=F, keepdims=True) * F(2.0)
    return ((a - b) + c).astype(F)


def quat_apply(q, v):
    xyz = q[:, :3]
    t = (np.cross(xyz, v) * F(2.0)).astype(v.dtype)
    return (v + q[:, 3:4] * t + np.cross(xyz, t)).astype(v.dtype)


def wrap_to_pi(a):
    """as the scripted reference runs: TorchScript's `%=` is fmod_, the truncated remainder (angles below -pi stay)"""
    two_pi = F(2 * np.pi)
    a = np.fmod(a, two_pi).astype(F)
    return (a - two_pi * (a > F(np.pi))).astype(F)


def get_heights(p, root):
    """get_heights (anymal_terrain.py:515-538) under mg_height_scan's rule (migym.h): the yaw rotation as a cosine and a
    sine, trunc then clip of both cell indices, the lower of the cell's two diagonal corners"""
    N = len(root)
    if p["table"] is None:
        return np.zeros((N, len(p["points"])), F)
    qz, qw = root[:, 5].astype(np.float64), root[:, 6].astype(np.float64)
    il = 1.0 / np.sqrt(qz * qz + qw * qw)
    z, w = qz * il, qw * il
    c, s = (w * w - z * z)[:, None], (2.0 * w * z)[:, None]
    px, py = p["points"][None, :, 0].astype(np.float64), p["points"][None, :, 1].astype(np.float64)
    X = (c * px - s * py) + root[:, 0:1]
    Y = (s * px + c * py) + root[:, 1:2]
    nx, ny = p["table"].shape
    with np.errstate(invalid="ignore"):
        ix = np.clip(np.nan_to_num(np.trunc((X - p["x0"]) / p["dx"]), nan=0.0, posinf=1e9, neginf=-1e9), 0, nx - 2)
        iy = np.clip(np.nan_to_num(np.trunc((Y - p["y0"]) / p["dx"]), nan=0.0, posinf=1e9, neginf=-1e9), 0, ny - 2)
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)
    return np.minimum(p["table"][ix, iy], p["table"][ix + 1, iy + 1]).astype(F)


def cell_margin(p, root):
    """how far, in cells, every scan point lies from the nearest cell edge (the golden generator's precondition)"""
    qz, qw = root[:, 5].astype(np.float64), root[:, 6].astype(np.float64)
    il = 1.0 / np.sqrt(qz * qz + qw * qw)
    z, w = qz * il, qw * il
    c, s = (w * w - z * z)[:, None], (2.0 * w * z)[:, None]
    px, py = p["points"][None, :, 0].astype(np.float64), p["points"][None, :, 1].astype(np.float64)
    fx = ((c * px - s * py) + root[:, 0:1] - float(p["x0"])) / float(p["dx"])
    fy = ((s * px + c * py) + root[:, 1:2] - float(p["y0"])) / float(p["dx"])
    return np.minimum(np.abs(fx - np.rint(fx)), np.abs(fy - np.rint(fy)))


def norm(x):
    return np.sqrt((x * x).sum(-1, dtype=F)).astype(F)


def update_terrain_level(p, st, e, frobenius_ids=None):
    """update_terrain_level for env e with the norm of its own commands; frobenius_ids: the reference's norm over all
    the envs that reset with it (for the generator's precondition and the deviation's test)"""
    d = st["root"][e, :2] - st["env_origins"][e, :2]
    dist = F(np.sqrt(F(d[0] * d[0]) + F(d[1] * d[1])))
    c = st["commands"][e, :2] if frobenius_ids is None else st["commands"][frobenius_ids, :2].ravel()
    cn = F(np.sqrt((c * c).sum(dtype=F)))
    level = int(st["terrain_levels"][e])
    level -= int(dist < F(F(cn * p["max_s"]) * F(0.25)))
    level += int(dist > F(p["env_length"] * F(0.5)))
    return max(level, 0) % p["env_rows"]


def reset_envs(p, st, env_ids, noise, update_levels=True, manual=False):
    """reset_idx (anymal_terrain.py:384-425); returns nothing, fills st["episode_out"] when env_ids is not empty"""
    env_ids = list(env_ids)
    if not env_ids:
        return
    for e in env_ids:
        u = noise[e].astype(F)
        st["dof"][e, :, 0] = p["default"] * (F(1.5 - 0.5) * u[C_POS:C_POS + 12] + F(0.5))
        st["dof"][e, :, 1] = F(0.1 - -0.1) * u[C_VEL:C_VEL + 12] + F(-0.1)
    if p["custom_origins"]:
        if update_levels and p["curriculum"]:
            levels = [update_terrain_level(p, st, e) for e in env_ids]
            for e, lv in zip(env_ids, levels):
                st["terrain_levels"][e] = lv
                st["env_origins"][e] = p["terrain_origins"][lv, st["terrain_types"][e]]
        for e in env_ids:
            u = noise[e].astype(F)
            st["root"][e] = p["base_init"]
            st["root"][e, :3] += st["env_origins"][e]
            st["root"][e, :2] += F(0.5 - -0.5) * u[C_ROOT:C_ROOT + 2] + F(-0.5)
    else:
        st["root"][env_ids] = p["base_init"]
    for e in env_ids:
        u = noise[e].astype(F)
        st["commands"][e, [0, 1, 3]] = p["cmd_span"] * u[C_CMD:C_CMD + 3] + p["cmd_lo"]
        st["commands"][e] *= F(norm(st["commands"][e, :2]) > F(0.25))
    st["feet_air_time"][env_ids] = 0
    st["progress"][env_ids] = 0
    st["reset"][env_ids] = 1
    if manual:
        st["last_actions"][env_ids] = 0
        st["last_dof_vel"][env_ids] = 0
    sums = st["episode_sums"][env_ids].astype(np.float64)
    st["episode_out"][:13] = (sums.mean(0) / float(p["max_s"])).astype(F)
    st["episode_sums"][env_ids] = 0
    st["episode_out"][13] = F(st["terrain_levels"].astype(np.float64).mean())


def post_step(p, st, ncf, actions, noise, push_now=False):
    """returns dict(obs, obs_clamped, rew, measured_heights); st holds everything else"""
    N = len(st["root"])
    act = np.clip(actions.astype(F), -p["clip_actions"], p["clip_actions"])
    ncf = ncf.astype(F)
    st["progress"] += 1
    root = st["root"]
    if push_now:
        root[:, 7:9] = F(1.0 - -1.0) * noise[:, C_PUSH:C_PUSH + 2].astype(F) + F(-1.0)
    q = root[:, 3:7]
    lin = quat_rotate_inverse(q, root[:, 7:10])
    ang = quat_rotate_inverse(q, root[:, 10:13])
    pg = quat_rotate_inverse(q, np.tile(np.array([0, 0, -1], F), (N, 1)))
    fwd = quat_apply(q, np.tile(np.array([1, 0, 0], F), (N, 1)))
    heading = np.arctan2(fwd[:, 1], fwd[:, 0]).astype(F)
    cmd = st["commands"]
    cmd[:, 2] = np.clip(F(0.5) * wrap_to_pi((cmd[:, 3] - heading).astype(F)), F(-1), F(1))
    # check_termination
    rst = norm(ncf[:, p["base"]]) > 1.0
    knee_contact = norm(ncf[:, p["knees"]]) > 1.0
    if not p["allow_knee"]:
        rst |= knee_contact.any(-1)
    rst |= st["progress"] >= p["max_episode_length"] - 1
    # compute_reward
    dof_pos, dof_vel = st["dof"][..., 0], st["dof"][..., 1]
    sq = np.square
    d = cmd[:, :2] - lin[:, :2]
    t = np.zeros((N, 13), F)
    t[:, 0] = np.exp(-(d * d).sum(-1, dtype=F) / F(0.25)) * p["rew"][0]
    t[:, 1] = sq(lin[:, 2]) * p["rew"][1]
    t[:, 2] = np.exp(-sq(cmd[:, 2] - ang[:, 2]) / F(0.25)) * p["rew"][2]
    t[:, 3] = sq(ang[:, :2]).sum(-1, dtype=F) * p["rew"][3]
    t[:, 4] = sq(pg[:, :2]).sum(-1, dtype=F) * p["rew"][4]
    t[:, 5] = sq(st["torques"]).sum(-1, dtype=F) * p["rew"][5]
    t[:, 6] = sq(st["last_dof_vel"] - dof_vel).sum(-1, dtype=F) * p["rew"][6]
    t[:, 7] = sq(root[:, 2] - F(0.52)) * p["rew"][7]
    feet = ncf[:, p["feet"]]
    contact = feet[..., 2] > 1.0
    first = (st["feet_air_time"] > 0.0) & contact
    st["feet_air_time"] += p["dt"]
    air = ((st["feet_air_time"] - F(0.5)) * first).sum(-1, dtype=F) * p["rew"][8]
    t[:, 8] = air * (norm(cmd[:, :2]) > F(0.1))
    st["feet_air_time"] *= ~contact
    t[:, 9] = knee_contact.sum(-1).astype(F) * p["rew"][9]
    stumble = (norm(feet[..., :2]) > 5.0) & (np.abs(feet[..., 2]) < 1.0)
    t[:, 10] = stumble.sum(-1).astype(F) * p["rew"][10]
    t[:, 11] = sq(st["last_actions"] - act).sum(-1, dtype=F) * p["rew"][11]
    t[:, 12] = np.abs(dof_pos[:, p["hips"]] - p["default"][p["hips"]]).sum(-1, dtype=F) * p["rew"][12]
    rew = t[:, 0]
    for k in (2, 1, 3, 4, 7, 5, 6, 9, 11, 8, 12, 10):   # anymal_terrain.py:362-363
        rew = (rew + t[:, k]).astype(F)
    raw = rew.copy()
    rew = np.maximum(rew, F(0)).astype(F)
    rew = (rew + p["rew_term"] * (rst & ~st["timeout"]).astype(F)).astype(F)
    st["episode_sums"] += t
    st["reset"][:] = rst
    base_cols = np.concatenate([lin * p["lin"], ang * p["ang"], pg], -1).astype(F)   # stale for the envs reset below
    reset_envs(p, st, np.nonzero(rst)[0], noise)
    heights = get_heights(p, root)
    hcols = (np.clip((root[:, 2:3] - F(0.5) - heights).astype(F), F(-1), F(1)) * p["hscale"]).astype(F)
    scale = np.array([p["lin"], p["lin"], p["ang"]], F)
    obs = np.concatenate([base_cols, cmd[:, :3] * scale, st["dof"][..., 0] * p["dof_pos"],
                          st["dof"][..., 1] * p["dof_vel"], hcols, act], -1).astype(F)
    if p["add_noise"]:
        obs = (obs + (F(2) * noise[:, C_OBS:].astype(F) - F(1)) * p["noise_vec"]).astype(F)
    st["last_actions"][:] = act
    st["last_dof_vel"][:] = st["dof"][..., 1]
    st["timeout"][:] = (st["progress"] >= p["max_episode_length"] - 1) & (st["reset"] != 0)
    return dict(obs=obs, obs_clamped=np.clip(obs, -p["clip_obs"], p["clip_obs"]), rew=rew, raw=raw,
                measured_heights=heights)


def close(x, ref):
    """the project's 1e-4 rule: |x - ref| <= 1e-4 max(1, |ref|)"""
    return np.abs(np.asarray(x, np.float64) - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))


# ---- the reference trace (tests/golden/trace_anymal_terrain.npz, written by tests/golden/make_anymal_terrain_golden.py)
@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN))
    for v in g.values():
        v.setflags(write=False)
    return g


def trace_cfg(N, episode_length_s, terminal_reward, rows, cols, env_length, **env):
    """the built-in config with the trace's settings: its episode length, knee contacts that terminate, a terminal
    reward, clips at 1 (actions) and 5 (observations), rows x cols maps of env_length metres; terrainType plane -- the trace's synthetic terrain is bound by the
    tests themselves (golden_terrain)"""
    from migym import configs
    over = {"env.learn.episodeLength_s": float(episode_length_s), "env.learn.allowKneeContacts": False,
            "env.learn.terminalReward": float(terminal_reward), "env.clipActions": CLIP_ACTIONS,
            "env.clipObservations": CLIP_OBS, "env.asset": {"modelTable": ANYMAL_JSON},
            "env.terrain.terrainType": "plane", "env.terrain.numLevels": int(rows), "env.terrain.numTerrains": int(cols),
            "env.terrain.mapLength": float(env_length), "env.terrain.mapWidth": float(env_length)}
    over.update({"env." + k: v for k, v in env.items()})
    return configs.task_config("AnymalTerrain", N, overrides=over)


def golden_cfg(N, **env):
    """the task config the trace was generated for (env overrides on top)"""
    g = golden()
    return trace_cfg(N, g["episode_length_s"], g["terminal_reward"], g["env_rows"], g["env_cols"], g["env_length"],
                     **env)


def task_cfg(N, **env):
    """the built-in AnymalTerrain config on the fixture table"""
    from migym import configs
    over = {"env.asset": {"modelTable": ANYMAL_JSON}}
    over.update({"env." + k: v for k, v in env.items()})
    return configs.task_config("AnymalTerrain", N, overrides=over)


def task_model(cfg):
    """(spec, packed model, sim params, terrain params) of the task as configured by ``cfg``"""
    from migym import model as M, taskdefs
    spec = taskdefs.anymal_terrain_spec(M.load_json(ANYMAL_JSON), cfg)
    sim_cfg = dict(cfg, env=dict(cfg["env"], plane=cfg["env"]["terrain"]))
    return spec, M.pack_model(spec), taskdefs.sim_params(sim_cfg, taskdefs.TASK_INFO["AnymalTerrain"][5], 1), \
        taskdefs.anymal_terrain_params(cfg, spec)


def golden_terrain(ap, N):
    """the synthetic terrain of the trace of N envs written into ``ap`` (but for the table's device pointer): returns
    (table in metres fp32, terrain_origins)"""
    g = golden()
    table = (g[f"N{N}_height_field_raw"].astype(F) * F(g["vertical_scale"])).astype(F)
    ap.hf_nx, ap.hf_ny = table.shape
    ap.hf_dx, ap.hf_x0, ap.hf_y0 = float(g["horizontal_scale"]), -float(g["border_size"]), -float(g["border_size"])
    ap.env_length, ap.env_rows, ap.env_cols = float(g["env_length"]), int(g["env_rows"]), int(g["env_cols"])
    ap.custom_origins, ap.curriculum = 1, 1
    return table, g[f"N{N}_terrain_origins"].astype(F)


def golden_state(g, N, t):
    """the task state step t of the trace starts from (copies)"""
    pre = f"N{N}_s{t}_"
    return {k: g[pre + k + "_in"].copy() for k in STATE_KEYS}


def golden_params(N):
    spec, mnp, sp, ap = task_model(golden_cfg(N))
    table, origins = golden_terrain(ap, N)
    return ap, params_from(ap, table, origins), table, origins
