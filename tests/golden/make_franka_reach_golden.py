#!/usr/bin/env python3
"""FrankaReachMA's post-physics step from the reference's own methods.

Run in the build container only (needs the reference checkout, MIGYM_REFERENCE):

    python tests/golden/make_franka_reach_golden.py

The task layer of ``FrankaReachMA`` (isaacgymenvs/tasks/franka_reach_MA.py) is plain torch, so its methods are
called here unmodified, bound to a stand-in ``self`` that holds only the attributes they read:
``post_physics_step`` (821-829) and through it ``reset_idx`` (616-679), ``_agent_ids_to_env_ids`` /
``_env_ids_to_agent_ids`` (875-889), ``_reset_init_cube_state`` (681-704), ``compute_observations`` (582-612) with
``_refresh`` / ``_update_states`` (519-568), and ``compute_reward`` -> ``compute_franka_reward`` (570-574, 928-960).
``gym`` is a stand-in whose every call is a no-op, ``gymtorch.unwrap_tensor`` the identity, and ``torch.rand`` is
wrapped to record every draw.  ``_get_franka_start_poses_rots`` (912-918) gives the base poses.  With T != A the
reference's ``_update_states`` cannot form its unused ``cubeA_pos_relative`` entry (shapes (N, T, 3) - (N, A, 3)); the
stand-in's cube tensor (CubeTensor) answers that one subtraction with an empty tensor, everything else is torch's.

For each configuration (A, T, N) in CONFIGS: 6 post-physics steps.  Before each step the post-simulate state is
written the way gym.simulate would leave it -- seeded random ``_q`` / ``_qd``, end-effector rows, hand contact force
rows (norms 0, just under and just over 0.1, never within 1e-3 of it) -- with seeded random actions (some beyond the
clip; VecTask.step's clamp is applied before they are handed over, vec_task.py step) and a reset mask that has envs
fully done, partly done and not done on top of what the previous step's reward set; ``progress`` starts so that some
agents reach max_episode_length - 1 within the six steps.  Recorded: the inputs, the draws in the (N, 3T+9) layout
[z of each cube (T) | xy of each cube (2T) | DOF noise (9)] (zero rows for envs that did not reset), and every output
after each step.  The fixture holds data only: tests/golden/trace_franka_reach_ma.npz.

Preconditions are asserted, so a comparison against this file cannot hide a flip: for every agent the nearest and
second-nearest cube distances differ by more than 1e-4 relative, and no reward lies within 1e-4 of the clip at 0 unless
it is far below it (a punished agent: at most -5 before the clip).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402

_refshim.install()
import isaacgymenvs.tasks.franka_reach_MA as ref  # noqa: E402
from isaacgymenvs.tasks.franka_reach_MA import FrankaReachMA  # noqa: E402

ref.gymtorch.unwrap_tensor = lambda t: t

CONFIGS = [(2, 2, 16), (3, 3, 8), (4, 2, 8), (1, 1, 8)]
STEPS = 6
MAX_EPISODE_LENGTH = 12
CLIP_ACTIONS, CLIP_OBS = 1.0, 5.0
START_POSITION_NOISE, FRANKA_DOF_NOISE = 0.25, 0.25
DEFAULT_DOF_POS = [0, 0.1963, 0, -2.6180, 0, 2.9416, 0.7854, 0.035, 0.035]   # franka_reach_MA.py:206-208
# the fixture table's joint limits (tests/golden/franka_panda.json; the URDF's)
DOF_LOWER = [-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973, 0.0, 0.0]
DOF_UPPER = [2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973, 0.04, 0.04]
NB, GRIP, HAND = 16, 15, 8   # rigid bodies per arm, panda_grip_site, panda_hand (the fixture table's order)


class NoGym:
    def __getattr__(self, name):
        return lambda *a, **k: None


class RandRecorder:
    """torch.rand, recording every draw in call order"""

    def __init__(self):
        self.real, self.draws = torch.rand, []

    def __call__(self, *a, **k):
        t = self.real(*a, **k)
        self.draws.append(t.clone())
        return t


class CubeTensor(torch.Tensor):
    """The cube tensor of a stand-in with T != A.  ``_update_states`` also forms ``cubeA_pos_relative`` =
    cube positions (N, T, 3) - eef positions (N, A, 3) (franka_reach_MA.py:548), an entry nothing reads and one that
    only broadcasts for T == A or T == 1: for that one subtraction this tensor yields an empty result instead of
    raising, so the method runs unmodified.  Every other operation is torch's own."""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        try:
            return super().__torch_function__(func, types, args, kwargs or {})
        except RuntimeError:
            if getattr(func, "__name__", "") in ("sub", "__sub__") and len(args) == 2 and \
                    args[0].shape[:1] == args[1].shape[:1] and args[0].shape[1] != args[1].shape[1]:
                return torch.empty(0)
            raise


def stand_in(A, T, N):
    s = types.SimpleNamespace(num_envs=N, num_agents=A, num_targets=T, device="cpu", viewer=None, debug_viz=False,
                              gym=NoGym(), sim=None, max_episode_length=MAX_EPISODE_LENGTH,
                              start_position_noise=START_POSITION_NOISE, start_rotation_noise=0.785,
                              franka_dof_noise=FRANKA_DOF_NOISE, reward_settings={"r_dist_scale": 0.1})
    for name in ("post_physics_step", "reset_idx", "_agent_ids_to_env_ids", "_env_ids_to_agent_ids",
                 "_reset_init_cube_state", "compute_observations", "compute_reward", "_refresh", "_update_states",
                 "_get_franka_start_poses_rots"):
        setattr(s, name, types.MethodType(getattr(FrankaReachMA, name), s))
    # the reference's env layout [table, stand, cubes, arms] (franka_reach_MA.py:374-424) for its index tensors
    s._cubeA_ids = list(range(2, 2 + T))
    s.frankas = [list(range(2 + T, 2 + T + A))]
    s._global_indices = torch.arange(N * (2 + T + A), dtype=torch.int32).view(N, -1)
    s._table_surface_pos = np.array([0.0, 0.0, 1.0]) + np.array([0, 0, 0.05 / 2])     # franka_reach_MA.py:338
    s.franka_default_dof_pos = torch.tensor(DEFAULT_DOF_POS, dtype=torch.float)
    s.franka_dof_lower_limits = torch.tensor(DOF_LOWER, dtype=torch.float)
    s.franka_dof_upper_limits = torch.tensor(DOF_UPPER, dtype=torch.float)
    s._root_state = torch.zeros(N, 2 + T + A, 13)
    s._cubeA_state = s._root_state[:, 2:2 + T, :]
    if T not in (1, A):
        s._cubeA_state = s._cubeA_state.as_subclass(CubeTensor)
    s._init_cubeA_state = torch.zeros(N, T, 13)
    s._dof_state = torch.zeros(N, A * 9, 2)
    s._q, s._qd = s._dof_state[..., 0], s._dof_state[..., 1]
    s._rigid_body_state = torch.zeros(N, A * NB, 13)
    s._eef_state = s._rigid_body_state[:, GRIP::NB, :]
    s._base_state = s._rigid_body_state[:, 0::NB, :]
    s._eef_lf_state = s._rigid_body_state[:, [12 + NB * k for k in range(A)], :]
    s._eef_rf_state = s._rigid_body_state[:, [14 + NB * k for k in range(A)], :]
    s._contact_forces = torch.zeros(N, A * NB, 3)
    s._hands_contact_forces = s._contact_forces[:, HAND::NB, :]
    s._pos_control = torch.zeros(N, A * 9)
    s._effort_control = torch.zeros_like(s._pos_control)
    s.states = {"cubeA_size": torch.ones(N, 1) * 0.050}                                # franka_reach_MA.py:282, 491
    s.obs_buf = torch.zeros(N * A, 10 + 3 * T + 3 * (A - 1))
    s.rew_buf = torch.zeros(N * A)
    s.reset_buf = torch.ones(N * A, dtype=torch.long)
    s.progress_buf = torch.zeros(N * A, dtype=torch.long)
    s.actions = torch.zeros(N * A, 6)
    return s


def run(A, T, N, rng):
    s = stand_in(A, T, N)
    n = N * A
    tag = f"A{A}T{T}_"
    out = {}
    # constants the task computes at setup, as the reference's expressions give them
    out[tag + "dof_noise_scale"] = np.float32(s.franka_dof_noise * 2.0)
    out[tag + "cube_xy_scale"] = np.float32(2.0 * s.start_position_noise)
    out[tag + "cube_z_base"] = (s._table_surface_pos[2] + s.states["cubeA_size"][:1] / 2).numpy().reshape(())
    p, r = s._get_franka_start_poses_rots(0.45)
    out[tag + "base_pos"], out[tag + "base_rot"] = p.numpy()[:A], r.numpy()[:A]
    # initial task state: cubes somewhere over the table, controls from an earlier episode
    s._cubeA_state[:, :, 0:2] = torch.from_numpy(rng.uniform(-0.25, 0.25, (N, T, 2)).astype(np.float32))
    s._cubeA_state[:, :, 2] = torch.from_numpy(rng.uniform(1.05, 1.55, (N, T)).astype(np.float32))
    s._cubeA_state[:, :, 6] = 1.0
    s._init_cubeA_state[:] = s._cubeA_state
    s._pos_control[:] = torch.from_numpy(rng.uniform(-1, 1, (N, A * 9)).astype(np.float32))
    s._effort_control[:] = torch.from_numpy(rng.uniform(-5, 5, (N, A * 9)).astype(np.float32))
    s.reset_buf[:] = 0
    s.progress_buf[:] = torch.from_numpy(rng.integers(MAX_EPISODE_LENGTH - 8, MAX_EPISODE_LENGTH - 2, n))
    for k in ("cube", "init_cube", "pos_control", "effort_control"):
        src = {"cube": s._cubeA_state, "init_cube": s._init_cubeA_state, "pos_control": s._pos_control,
               "effort_control": s._effort_control}[k]
        out[tag + k + "_0"] = src.numpy().copy()
    lo, hi = np.array(DOF_LOWER), np.array(DOF_UPPER)
    reached = False
    for t in range(STEPS):
        # what gym.simulate leaves: DOF state, the grip sites' rows, the hands' contact forces
        q = (lo + (hi - lo) * rng.uniform(0, 1, (N, A, 9))).astype(np.float32).reshape(N, A * 9)
        qd = rng.uniform(-2, 2, (N, A * 9)).astype(np.float32)
        eef = np.zeros((N, A, 13), np.float32)
        eef[..., 0:2] = rng.uniform(-0.5, 0.5, (N, A, 2))
        eef[..., 2] = rng.uniform(1.0, 1.7, (N, A))
        quat = rng.normal(0, 1, (N, A, 4))
        eef[..., 3:7] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
        eef[..., 7:13] = rng.uniform(-1, 1, (N, A, 6))
        direc = rng.normal(0, 1, (N, A, 3))
        direc /= np.linalg.norm(direc, axis=-1, keepdims=True)
        kind = rng.integers(0, 4, (N, A))           # 0, 1: no force | 2: just under 0.1 | 3: just over
        mag = np.where(kind == 2, rng.uniform(0.05, 0.098, (N, A)),
                       np.where(kind == 3, rng.uniform(0.102, 0.5, (N, A)), 0.0))
        force = (direc * mag[..., None]).astype(np.float32)
        fn = np.linalg.norm(force.astype(np.float64), axis=-1)
        assert (np.abs(fn - 0.1) > 1e-3).all()
        actions = rng.uniform(-1.5, 1.5, (n, 6)).astype(np.float32)
        # the reset mask: the previous reward's flags plus a random ~40 % of the agents, with env 0 fully done, env 1
        # all but its last agent (partly done: the AND filter must leave it alone, flags included) and env 2 not done
        forced = (rng.random(n) < 0.4).astype(np.int64)
        reset_in = np.maximum(s.reset_buf.numpy(), forced)
        reset_in[0:2 * A] = 1
        if A > 1:
            reset_in[2 * A - 1] = 0
        reset_in[2 * A:3 * A] = 0
        s._q[:] = torch.from_numpy(q)
        s._qd[:] = torch.from_numpy(qd)
        s._eef_state[:] = torch.from_numpy(eef)
        s._hands_contact_forces[:] = torch.from_numpy(force)
        s.reset_buf[:] = torch.from_numpy(reset_in)
        s.actions = torch.clamp(torch.from_numpy(actions), -CLIP_ACTIONS, CLIP_ACTIONS)   # VecTask.step's clamp
        progress_in = s.progress_buf.numpy().copy()
        rec = RandRecorder()
        torch.rand = rec
        try:
            s.post_physics_step()
        finally:
            torch.rand = rec.real
        # the draws, in the (N, 3T+9) layout, at the rows of the envs that reset
        env_ids = FrankaReachMA._agent_ids_to_env_ids(s, torch.from_numpy(np.nonzero(reset_in)[0])).numpy()
        noise = np.zeros((N, 3 * T + 9), np.float32)
        if len(np.nonzero(reset_in)[0]):
            assert [tuple(d.shape) for d in rec.draws] == [(len(env_ids), T), (len(env_ids), T, 2), (len(env_ids), 9)]
            noise[env_ids, :T] = rec.draws[0].numpy()
            noise[env_ids, T:3 * T] = rec.draws[1].numpy().reshape(len(env_ids), 2 * T)
            noise[env_ids, 3 * T:] = rec.draws[2].numpy()
        else:
            assert not rec.draws
        per_env = reset_in.reshape(N, A).sum(1)
        assert (per_env == A).any() and (per_env == 0).any() and (A == 1 or ((per_env > 0) & (per_env < A)).any())
        # preconditions of a bit-level comparison
        c = s._cubeA_state[:, :, :3].numpy().astype(np.float64)
        dist = np.sort(np.linalg.norm(c[:, None] - eef[:, :, None, :3].astype(np.float64), axis=-1), axis=-1)
        if T > 1:
            assert ((dist[..., 1] - dist[..., 0]) > 1e-4 * dist[..., 1]).all(), "nearest / second-nearest too close"
        rew = s.rew_buf.numpy()
        punished = fn.reshape(-1) >= 0.1
        assert (rew[~punished] > 1e-4).all() and (rew[punished] == 0).all()
        d0 = dist[..., 0].reshape(-1)
        raw = 1.0 / (0.5 + d0 * d0) - 0.01 * (np.clip(actions, -1, 1).astype(np.float64) ** 2).sum(-1) + 1.0 - 10.0
        assert (raw[punished] < -5.0).all()
        reached = reached or bool((s.progress_buf.numpy() >= MAX_EPISODE_LENGTH - 1).any())
        pre = f"{tag}s{t}_"
        out.update({pre + "q_in": q, pre + "qd_in": qd, pre + "eef": eef, pre + "hand_force": force,
                    pre + "actions": actions, pre + "reset_in": reset_in, pre + "progress_in": progress_in,
                    pre + "noise": noise, pre + "obs": s.obs_buf.numpy().copy(), pre + "rew": rew.copy(),
                    pre + "reset": s.reset_buf.numpy().copy(), pre + "progress": s.progress_buf.numpy().copy(),
                    pre + "cube": s._cubeA_state.numpy().copy(), pre + "init_cube": s._init_cubeA_state.numpy().copy(),
                    pre + "q": s._q.numpy().copy(), pre + "qd": s._qd.numpy().copy(),
                    pre + "pos_control": s._pos_control.numpy().copy(),
                    pre + "effort_control": s._effort_control.numpy().copy()})
    assert reached, "no agent reached max_episode_length - 1"
    return out


def main():
    torch.manual_seed(20261020)
    rng = np.random.default_rng(20261020)
    out = {"configs": np.array(CONFIGS, np.int32), "steps": np.int32(STEPS),
           "max_episode_length": np.int32(MAX_EPISODE_LENGTH), "clip_actions": np.float32(CLIP_ACTIONS),
           "clip_obs": np.float32(CLIP_OBS), "start_position_noise": np.float32(START_POSITION_NOISE),
           "franka_dof_noise": np.float32(FRANKA_DOF_NOISE), "default_dof_pos": np.array(DEFAULT_DOF_POS, np.float32),
           "dof_lower": np.array(DOF_LOWER, np.float32), "dof_upper": np.array(DOF_UPPER, np.float32)}
    for A, T, N in CONFIGS:
        out.update(run(A, T, N, rng))
    path = os.path.join(HERE, "trace_franka_reach_ma.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
