"""Quadcopter's task layer restated in numpy fp32, and the reference trace it is held to (tests/test_quadcopter_host.py);
tests/test_gpu_quadcopter.py replays the same trace through mg_quadcopter_pre / mg_quadcopter_post.

The trace, tests/golden/trace_quadcopter.npz, is written by tests/golden/make_quadcopter_golden.py from the reference's
own unmodified methods.  Each operation below is one fp32 operation of the reference, in its order: a Python float
times a tensor is the float rounded to fp32 first, then an fp32 product.
"""
import functools
import math
import os

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "trace_quadcopter.npz")
STATE_KEYS = ("dof_position_targets", "thrusts", "forces", "root_states", "dof_states")
ROTORS = [2, 4, 6, 8]


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN))
    for v in g.values():
        v.setflags(write=False)
    return g


def golden_cfg(N):
    """the task config the trace was generated for"""
    from migym import configs
    g = golden()
    return configs.task_config("Quadcopter", N, overrides={"env.maxEpisodeLength": int(g["max_episode_length"])})


def params_from(qp):
    """the constants of an _abi.QuadcopterParams as numpy fp32"""
    return dict(dof_step=F(qp.dof_step), thrust_step=F(qp.thrust_step), lower=np.array(qp.dof_lower[:], F),
                upper=np.array(qp.dof_upper[:], F), thrust_lower=F(qp.thrust_lower), thrust_upper=F(qp.thrust_upper),
                init_root=np.array(qp.init_root[:], F), init_dof=np.array(qp.init_dof[:], F).reshape(8, 2),
                clip_actions=F(qp.clip_actions), clip_obs=F(qp.clip_obs), max_episode_length=int(qp.max_episode_length))


def close(x, ref):
    """the project's 1e-4 rule: |x - ref| <= 1e-4 max(1, |ref|)"""
    return np.abs(x.astype(np.float64) - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))


def rand(lower, upper, u):
    """torch_rand_float: (upper - lower) * u + lower, the span a Python float"""
    return F(upper - lower) * u + F(lower)


def reset_envs(p, st, ids, noise):
    """reset_idx (quadcopter.py:280-299) on the dict st, in place; noise: (N, 11) rows by env"""
    st["dof_states"][ids] = p["init_dof"]
    st["root_states"][ids] = p["init_root"]
    st["root_states"][ids, 0] += rand(-1.5, 1.5, noise[ids, 0])
    st["root_states"][ids, 1] += rand(-1.5, 1.5, noise[ids, 1])
    st["root_states"][ids, 2] += rand(-0.2, 1.5, noise[ids, 2])
    st["dof_states"][ids, :, 0] = rand(-0.2, 0.2, noise[ids, 3:11])
    st["dof_states"][ids, :, 1] = 0.0
    st["reset"][ids] = 0
    st["progress"][ids] = 0


def pre_step(p, st, actions, noise):
    """pre_physics_step (quadcopter.py:301-330) with VecTask.step's action clamp before it; returns the clamped
    actions"""
    ids = np.nonzero(st["reset"])[0]
    if len(ids):
        reset_envs(p, st, ids, noise)
    a = np.clip(actions, -p["clip_actions"], p["clip_actions"]).astype(F)
    st["dof_position_targets"] += p["dof_step"] * a[:, 0:8]
    st["dof_position_targets"][:] = np.maximum(np.minimum(st["dof_position_targets"], p["upper"]), p["lower"])
    st["thrusts"] += p["thrust_step"] * a[:, 8:12]
    st["thrusts"][:] = np.maximum(np.minimum(st["thrusts"], p["thrust_upper"]), p["thrust_lower"])
    st["forces"][:, ROTORS, 2] = st["thrusts"]
    st["thrusts"][ids] = 0.0
    st["forces"][ids] = 0.0
    st["dof_position_targets"][ids] = st["dof_states"][ids, :, 0]
    return a


def observe(root, dof):
    obs = np.zeros((len(root), 21), F)
    obs[:, 0] = (F(0.0) - root[:, 0]) / F(3)
    obs[:, 1] = (F(0.0) - root[:, 1]) / F(3)
    obs[:, 2] = (F(1.0) - root[:, 2]) / F(3)
    obs[:, 3:7] = root[:, 3:7]
    obs[:, 7:10] = root[:, 7:10] / F(2)
    obs[:, 10:13] = root[:, 10:13] / F(math.pi)
    obs[:, 13:21] = dof[:, :, 0]
    return obs


def reward(p, root, progress):
    """compute_quadcopter_reward (quadcopter.py:386-418): (reward, reset)"""
    x, y, z = root[:, 0], root[:, 1], root[:, 2]
    dz = F(1) - z
    dist = np.sqrt(x * x + y * y + dz * dz)
    pos = F(1.0) / (F(1.0) + dist * dist)
    qv, qw = root[:, 3:6], root[:, 6]
    ez = np.zeros((len(root), 3), F)
    ez[:, 2] = 1
    a = ez * (F(2.0) * qw ** 2 - F(1.0))[:, None]
    b = np.cross(qv, ez).astype(F) * qw[:, None] * F(2.0)
    c = qv * (qv * ez).sum(1, dtype=F)[:, None] * F(2.0)
    ups = a + b + c
    tilt = np.abs(F(1) - ups[:, 2])
    up = F(1.0) / (F(1.0) + tilt * tilt)
    spin = np.abs(root[:, 12])
    spin_r = F(1.0) / (F(1.0) + spin * spin)
    rew = pos + pos * (up + spin_r)
    die = (dist > F(3.0)) | (z < F(0.3))
    reset = np.where(progress >= p["max_episode_length"] - 1, 1, die.astype(np.int64))
    return rew.astype(F), reset, dist


def post_step(p, st):
    """post_physics_step + the VecTask.step tail on the post-simulate state in st: (obs, clamped obs, timeout)"""
    st["progress"] += 1
    obs = observe(st["root_states"], st["dof_states"])
    st["rew"], st["reset"], _ = reward(p, st["root_states"], st["progress"])
    timeout = (st["progress"] >= p["max_episode_length"] - 1) & (st["reset"] != 0)
    return obs, np.clip(obs, -p["clip_obs"], p["clip_obs"]), timeout


def task_model(cfg):
    """(spec, packed model, sim params, quadcopter params) of the task as configured by ``cfg``"""
    from migym import model as M, taskdefs
    spec = taskdefs.quadcopter_spec(M.quadcopter_model())
    return spec, M.pack_model(spec), taskdefs.sim_params(cfg, taskdefs.QUADCOPTER_MAX_CONTACTS, 1), \
        taskdefs.quadcopter_params(cfg, spec)


def trace_state0(g, N):
    st = {k: g[f"N{N}_{k}_0"].copy() for k in STATE_KEYS}
    st["reset"], st["progress"] = np.zeros(N, np.int64), np.zeros(N, np.int64)
    return st


def uniform_host(seed, env, counter, col):
    """the device counter RNG's host twin (pyoracle.uniform)"""
    import pyoracle as O
    return O.uniform(seed, env, counter, col)
