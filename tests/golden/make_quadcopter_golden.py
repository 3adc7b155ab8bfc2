#!/usr/bin/env python3
"""The quadcopter's model table from the MJCF the reference writes at run time.

Run in the build container only (needs the reference checkout, MIGYM_REFERENCE):

    python tests/golden/make_quadcopter_golden.py

The reference ships no quadcopter asset: ``Quadcopter._create_quadcopter_asset`` (isaacgymenvs/tasks/quadcopter.py:
121-202) writes ``quadcopter.xml`` into the working directory when the task starts.  That method is called here
unmodified, on a stand-in ``self`` (it reads no attribute), in a temporary directory, with the two things it needs of
the closed wheel stood in for: ``gymapi.Quat.from_axis_angle`` / ``Quat.rotate`` (a unit quaternion about an axis, and
the rotation of a Vec3 by it) and ``gymutil._indent_xml`` (whitespace only: a no-op).  The file it writes goes through
``migym.model.load_mjcf`` unchanged, and the table that makes is the fixture tests/golden/quadcopter.json (data only):
9 nodes, 9 bodies (chassis, then rotor_arm i, rotor i for i = 0..3), 8 hinges limited to +-30 degrees, one cylinder
or sphere geom per body.  migym.model.quadcopter_model builds the same table from the named dimensions
(tests/test_quadcopter_host.py holds it to this file).

The task layer of ``Quadcopter`` is plain torch, so its methods are called unmodified too, bound to a stand-in ``self``
that holds only the attributes they read: ``pre_physics_step`` (301-330) and through it ``reset_idx`` (280-299),
``post_physics_step`` (332-340) and through it ``compute_observations`` (359-370) and ``compute_reward`` (372-379) ->
``compute_quadcopter_reward`` (386-418).  ``gym`` is a stand-in whose calls do nothing (the state tensors are written in
place), ``gymtorch.unwrap_tensor`` is the identity, and the module's ``torch_rand_float`` is replaced by a recorder that
evaluates the same expression, ``(upper - lower) * u + lower``, on a recorded ``u = torch.rand(shape)``.  ``dt`` is a C
float, as ``gymapi.SimParams.dt`` is; maxEpisodeLength is 8, so that time-outs occur within six steps.

Two traces, N = 6 and N = 67 envs, 6 control steps each, from seeded control tensors in mid-rollout.  Each step: seeded
actions (some beyond the clip; VecTask.step's clamp is applied before they are handed over) and a reset mask on top of
what the previous step's reward set; then the post-simulate state written the way gym.simulate would leave it (near
the target, far from it, low, or near and slow; some observations past the clip).  Recorded: the inputs, the draws in
the (N, 11) layout [x | y | z | dof position 8] (zero rows for envs that did not reset), every tensor after
pre_physics_step and every output after post_physics_step with the VecTask.step tail (time-outs, clamped
observations).  The fixture holds data only: tests/golden/trace_quadcopter.npz.

Preconditions are asserted: every branch of the reset predicate fires (distance, height, time-out, none); no
target_dist lies within 1e-3 of 3 and no z within 1e-3 of 0.3; actions beyond the clip are present; some thrusts and
targets reach each clamp.
"""
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402

_refshim.install()
import isaacgym  # noqa: E402  (the shim's stand-in modules)

gymapi, gymutil = isaacgym.gymapi, isaacgym.gymutil


class Quat(gymapi.Quat):
    @staticmethod
    def from_axis_angle(axis, angle):
        s = math.sin(0.5 * angle)
        return Quat(axis.x * s, axis.y * s, axis.z * s, math.cos(0.5 * angle))

    def rotate(self, v):
        # v + 2 w (q x v) + 2 q x (q x v)
        qx, qy, qz, w = self.x, self.y, self.z, self.w
        cx, cy, cz = qy * v.z - qz * v.y, qz * v.x - qx * v.z, qx * v.y - qy * v.x
        dx, dy, dz = qy * cz - qz * cy, qz * cx - qx * cz, qx * cy - qy * cx
        return gymapi.Vec3(v.x + 2 * (w * cx + dx), v.y + 2 * (w * cy + dy), v.z + 2 * (w * cz + dz))


gymapi.Quat = Quat
gymutil._indent_xml = lambda root: None
import isaacgymenvs.tasks.quadcopter as ref  # noqa: E402
from isaacgymenvs.tasks.quadcopter import Quadcopter  # noqa: E402

ref.gymtorch.unwrap_tensor = lambda t: t

sys.path.insert(0, os.path.join(HERE, "..", "..", "isaacgymenvs-ma_amd"))
from migym import model as M  # noqa: E402


SIZES, STEPS = [6, 67], 6
DT, MAX_EPISODE_LENGTH, CLIP_ACTIONS, CLIP_OBS = 0.01, 8, 1.0, 5.0    # Quadcopter.yaml, but for the episode length
TRACE = os.path.join(HERE, "trace_quadcopter.npz")


class Gym:
    """every gym call of the task layer is a no-op here: the state tensors are written in place"""

    def __getattr__(self, name):
        return lambda *a, **k: None


class RandRecorder:
    """the module's torch_rand_float, keeping each draw's raw U(0,1)"""

    def __init__(self):
        self.draws = []

    def __call__(self, lower, upper, shape, device):
        u = torch.rand(*shape, device=device)
        self.draws.append(u.clone())
        return (upper - lower) * u + lower


def stand_in(N, spec, rng):
    s = types.SimpleNamespace(num_envs=N, device="cpu", sim=None, viewer=None, debug_viz=False, gym=Gym(),
                              dt=float(np.float32(DT)), max_episode_length=MAX_EPISODE_LENGTH)
    for name in ("pre_physics_step", "post_physics_step", "reset_idx", "compute_observations", "compute_reward"):
        setattr(s, name, types.MethodType(getattr(Quadcopter, name), s))
    s.root_states = torch.zeros(N, 13)
    s.root_states[:, 2], s.root_states[:, 6] = 1.0, 1.0          # default_pose.p.z = 1 (quadcopter.py:236-237)
    s.root_tensor = s.root_states
    s.root_positions, s.root_quats = s.root_states[..., 0:3], s.root_states[..., 3:7]
    s.root_linvels, s.root_angvels = s.root_states[..., 7:10], s.root_states[..., 10:13]
    s.dof_states = torch.zeros(N, 8, 2)
    s.dof_state_tensor = s.dof_states
    s.dof_positions, s.dof_velocities = s.dof_states[..., 0], s.dof_states[..., 1]
    s.initial_root_states, s.initial_dof_states = s.root_states.clone(), s.dof_states.clone()
    s.dof_lower_limits = torch.tensor([n.lower for n in spec.nodes[1:]], dtype=torch.float)
    s.dof_upper_limits = torch.tensor([n.upper for n in spec.nodes[1:]], dtype=torch.float)
    s.thrust_lower_limits, s.thrust_upper_limits = torch.zeros(4), 2 * torch.ones(4)
    # control tensors in mid-rollout: targets over the whole range, so that both clamps are reached within six steps
    s.dof_position_targets = torch.from_numpy(rng.uniform(-0.5, 0.5, (N, 8)).astype(np.float32))
    s.thrusts = torch.from_numpy(rng.uniform(0, 2, (N, 4)).astype(np.float32))
    s.forces = torch.zeros(N, 9, 3)
    s.forces[:, [2, 4, 6, 8], 2] = s.thrusts
    s.all_actor_indices = torch.arange(N, dtype=torch.int32)
    s.obs_buf, s.rew_buf = torch.zeros(N, 21), torch.zeros(N)
    s.reset_buf = torch.ones(N, dtype=torch.long)
    s.progress_buf = torch.zeros(N, dtype=torch.long)
    return s


def run(N, spec, rng):
    s = stand_in(N, spec, rng)
    tag, out = f"N{N}_", {}
    n = lambda t: t.numpy().copy()   # noqa: E731
    for k in ("dof_position_targets", "thrusts", "forces", "root_states", "dof_states"):
        out[tag + k + "_0"] = n(getattr(s, k))
    s.reset_buf[:] = 0
    s.progress_buf[:] = torch.from_numpy(rng.integers(0, MAX_EPISODE_LENGTH - 1, N))
    seen = dict(dist=False, low=False, timeout=False, none=False)
    clamps = dict(tgt_lo=False, tgt_hi=False, thr_lo=False, thr_hi=False, beyond_clip=False)
    for t in range(STEPS):
        key = lambda name: f"{tag}t{t}_{name}"   # noqa: E731
        actions = rng.uniform(-1.5, 1.5, (N, 12)).astype(np.float32)
        clamps["beyond_clip"] |= bool((np.abs(actions) > CLIP_ACTIONS).any())
        forced = (rng.random(N) < 0.3).astype(np.int64)
        reset_in = np.maximum(n(s.reset_buf), forced)
        reset_in[0], reset_in[2 % N] = 1, 0
        s.reset_buf[:] = torch.from_numpy(reset_in)
        out[key("actions")], out[key("reset_in")], out[key("progress_in")] = actions, reset_in, n(s.progress_buf)
        rec = RandRecorder()
        ref.torch_rand_float = rec
        clamped = torch.clamp(torch.from_numpy(actions), -CLIP_ACTIONS, CLIP_ACTIONS)    # VecTask.step
        s.pre_physics_step(clamped)
        ids = np.nonzero(reset_in)[0]
        noise = np.zeros((N, 11), np.float32)
        if len(ids):
            assert [tuple(d.shape) for d in rec.draws] == [(len(ids), 1)] * 3 + [(len(ids), 8)]
            noise[ids] = torch.cat(rec.draws, dim=1).numpy()
        out[key("noise")] = noise
        for k in ("dof_position_targets", "thrusts", "forces", "root_states", "dof_states", "reset_buf", "progress_buf"):
            out[key("pre_" + k)] = n(getattr(s, k))
        tg, th = n(s.dof_position_targets), n(s.thrusts)
        lo, hi = n(s.dof_lower_limits), n(s.dof_upper_limits)
        clamps["tgt_lo"] |= bool((tg == lo).any())
        clamps["tgt_hi"] |= bool((tg == hi).any())
        clamps["thr_lo"] |= bool(((th == 0.0) & (reset_in == 0)[:, None]).any())
        clamps["thr_hi"] |= bool((th == 2.0).any())
        # what gym.simulate leaves: per env one of: near the target | far from it | low | near and slow
        kind = (np.arange(N) + t) % 4
        root = np.zeros((N, 13), np.float32)
        root[:, 0:2] = rng.uniform(-1.2, 1.2, (N, 2))
        root[:, 2] = rng.uniform(0.5, 2.0, N)
        far = kind == 1
        root[far, 0] = rng.uniform(3.2, 5.0, far.sum()) * rng.choice([-1.0, 1.0], far.sum())
        low = kind == 2
        root[low, 2] = rng.uniform(0.0, 0.29, low.sum())
        quat = rng.normal(0, 1, (N, 4)) * np.array([0.3, 0.3, 0.3, 1.0])
        root[:, 3:7] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
        root[:, 7:13] = rng.uniform(-8, 8, (N, 6)) * np.where(kind == 3, 0.05, 1.0)[:, None]   # some obs past the clip
        dof = np.zeros((N, 8, 2), np.float32)
        dof[..., 0], dof[..., 1] = rng.uniform(-0.5, 0.5, (N, 8)), rng.uniform(-10, 10, (N, 8))
        r64 = root.astype(np.float64)
        dist = np.sqrt(r64[:, 0] ** 2 + r64[:, 1] ** 2 + (1 - r64[:, 2]) ** 2)
        assert (np.abs(dist - 3.0) > 1e-3).all() and (np.abs(r64[:, 2] - 0.3) > 1e-3).all()
        s.root_states[:] = torch.from_numpy(root)
        s.dof_states[:] = torch.from_numpy(dof)
        out[key("sim_root_states")], out[key("sim_dof_states")] = root, dof
        s.post_physics_step()
        progress = n(s.progress_buf)
        late = progress >= MAX_EPISODE_LENGTH - 1
        reset = n(s.reset_buf)
        timeout = late & (reset != 0)                                   # vec_task.py:396
        seen["dist"] |= bool((dist > 3).any())
        seen["low"] |= bool((root[:, 2] < 0.3).any())
        seen["timeout"] |= bool((late & (dist <= 3) & (root[:, 2] >= 0.3)).any())
        seen["none"] |= bool((reset == 0).any())
        assert ((dist > 3) | (root[:, 2] < 0.3) | late).astype(np.int64).tolist() == reset.tolist()
        obs = n(s.obs_buf)
        out[key("obs")], out[key("obs_clamped")] = obs, np.clip(obs, -CLIP_OBS, CLIP_OBS)
        out[key("rew")], out[key("reset")], out[key("progress")], out[key("timeout")] = n(s.rew_buf), reset, progress, timeout
    assert all(seen.values()), seen
    assert all(clamps.values()), clamps
    return out


def traces(spec):
    torch.manual_seed(0)
    rng = np.random.default_rng(2024)
    out = dict(dt=np.float32(DT), max_episode_length=np.int64(MAX_EPISODE_LENGTH), clip_actions=np.float32(CLIP_ACTIONS),
               clip_obs=np.float32(CLIP_OBS), steps=np.int64(STEPS), sizes=np.array(SIZES))
    for N in SIZES:
        out.update(run(N, spec, rng))
    np.savez_compressed(TRACE, **out)
    print(TRACE, len(out), "arrays,", os.path.getsize(TRACE), "bytes")


def main():
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            Quadcopter._create_quadcopter_asset(object())
            spec = M.load_mjcf(os.path.join(td, "quadcopter.xml"), "quadcopter")
        finally:
            os.chdir(cwd)
    assert (len(spec.nodes), len(spec.bodies), spec.fixed_base) == (9, 9, 0)
    assert [b.name for b in spec.bodies] == ["chassis"] + [f"{p}{i}" for i in range(4) for p in ("rotor_arm", "rotor")]
    assert all(n.limited and abs(n.upper - math.radians(30)) < 1e-12 and n.lower == -n.upper for n in spec.nodes[1:])
    assert abs(spec.total_mass() - 0.25154) < 1e-5
    out = os.path.join(HERE, "quadcopter.json")
    spec.to_json(out)
    print(out, "nodes", len(spec.nodes), "mass", spec.total_mass())
    traces(spec)


if __name__ == "__main__":
    main()
